"""The pure-host calls of the C ABI: parameter algebra, the text front half, planning and the arithmetic around the
measurements and transforms.  None of them needs a device (device_count asks whether there is one)."""
import ctypes as C

import numpy as np

from ._abi import (DYN_POINTS, LEVEL_ACTIVE_FLOOR_DB, LEVEL_FRAME, NUM_FORMANTS, OK, PHONEME_DTYPE, TRUE_PEAK_PHASES,
                   TRUE_PEAK_TAPS, NodeShard, PlanBlock, Rule, SynthesisElem, Voice, _arr, _check, _ptr, load)


# ---- host-side parameter algebra -------------------------------------------
def voice_generic(sample_rate=None):
    """voices::generic() (src/voices/generic.rs:5); sample_rate != None gives the
    resampled variant of SURVEY.md §8d."""
    v = Voice()
    if sample_rate is None:
        load().grail_voice_generic(C.byref(v))
    else:
        load().grail_voice_generic_at(C.byref(v), C.c_float(sample_rate))
    return v


def elem_new_phoneme(freq, bw, smooth, turb, breath, amp):
    """SynthesisElem::new_phoneme == MKPHON (src/lib.rs:381, src/voices/mod.rs:7)."""
    e = SynthesisElem()
    arrs = [(C.c_float * NUM_FORMANTS)(*[float(x) for x in a])
            for a in (freq, bw, smooth, turb, breath, amp)]
    load().grail_elem_new_phoneme(C.byref(e), *arrs)
    return e


def elem_resample(elem, old_rate, new_rate):
    e = SynthesisElem.from_buffer_copy(bytes(elem))
    load().grail_elem_resample(C.byref(e), C.c_float(old_rate), C.c_float(new_rate))
    return e


def elem_silent():
    e = SynthesisElem()
    load().grail_elem_silent(C.byref(e))
    return e


def elem_blend(a, b, alpha):
    e = SynthesisElem()
    load().grail_elem_blend(C.byref(e), C.byref(a), C.byref(b), C.c_float(alpha))
    return e


def shard_range(n_utt, rank, world):
    b, e = C.c_uint64(), C.c_uint64()
    load().grail_shard_range(n_utt, rank, world, C.byref(b), C.byref(e))
    return b.value, e.value


def node_shard_of(seg_offsets, index, n_devices):
    """(NodeShard, rebased seg_offsets) of device slot `index` out of n_devices: the view a node call hands to that
    device's grail_synthesize_batch (grail_node_shard_of; pure host arithmetic, no GPU)."""
    offs = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
    n_utt = len(offs) - 1
    u32p = C.POINTER(C.c_uint32)
    sh = NodeShard()
    _check(load().grail_node_shard_of(offs.ctypes.data_as(u32p), n_utt, index, n_devices, C.byref(sh), None, 0))
    rebased = np.zeros(sh.rows + 1, dtype=np.uint32)
    _check(load().grail_node_shard_of(offs.ctypes.data_as(u32p), n_utt, index, n_devices, C.byref(sh),
                                      rebased.ctypes.data_as(u32p), len(rebased)))
    return sh, rebased


def voices_blob(voices):
    """The broadcast payload: the raw grail_voice[] bytes."""
    return b"".join(bytes(v) for v in voices)


def voices_from_blob(blob):
    n = len(blob) // C.sizeof(Voice)
    assert n * C.sizeof(Voice) == len(blob)
    return [Voice.from_buffer_copy(blob[i * C.sizeof(Voice):(i + 1) * C.sizeof(Voice)])
            for i in range(n)]


def segments(seq):
    a = np.zeros(len(seq), dtype=PHONEME_DTYPE)
    for i, s in enumerate(seq):
        a[i] = tuple(s)
    return a


# ---- text front half ---------------------------------------------------------
def make_rules(rule_list):
    """[(string, [phonemes...]), ...] -> (Rule array, keepalive list)."""
    keep = []
    arr = (Rule * len(rule_list))()
    for i, (st, ph) in enumerate(rule_list):
        cps = (C.c_uint32 * max(len(st), 1))(*[ord(ch) for ch in st])
        pp = (C.c_int32 * max(len(ph), 1))(*ph)
        keep += [cps, pp]
        arr[i].string = C.cast(cps, C.POINTER(C.c_uint32))
        arr[i].string_len = len(st)
        arr[i].phonemes = C.cast(pp, C.POINTER(C.c_int32))
        arr[i].n_phonemes = len(ph)
    return arr, keep


def transcribe(text, rule_list, case_sensitive=False, leading_silence=False):
    """Transcriber (src/lib.rs:1116); leading_silence=True is .transcribe() (:1201)."""
    arr, keep = make_rules(rule_list)
    cps = (C.c_uint32 * max(len(text), 1))(*[ord(ch) for ch in text])
    cap = 4 * len(text) + 8
    out = (C.c_int32 * cap)()
    n = C.c_uint32()
    _check(load().grail_transcribe(cps, len(text), arr, len(rule_list), int(case_sensitive),
                                   int(leading_silence), out, cap, C.byref(n)))
    return list(out[: n.value])


def language_generic():
    """languages::generic() as [(string, [phonemes])], case_sensitive."""
    rules = C.POINTER(Rule)()
    cs = C.c_int()
    n = load().grail_language_generic(C.byref(rules), C.byref(cs))
    out = []
    for i in range(n):
        r = rules[i]
        out.append(("".join(chr(r.string[k]) for k in range(r.string_len)),
                    [r.phonemes[k] for k in range(r.n_phonemes)]))
    return out, bool(cs.value)


def text_to_phoneme_elems(voice, text):
    n = C.c_uint32()
    _check(load().grail_text_to_phoneme_elems(C.byref(voice), text.encode("utf-8"), None, 0,
                                              C.byref(n)))
    a = np.zeros(max(n.value, 1), dtype=PHONEME_DTYPE)
    _check(load().grail_text_to_phoneme_elems(C.byref(voice), text.encode("utf-8"), a.ctypes.data,
                                              n.value, C.byref(n)))
    return a[: n.value]


def wav_write_i16(path, pcm, sample_rate):
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    _check(load().grail_wav_write_i16(path.encode(), pcm.ctypes.data, len(pcm), int(sample_rate)))


def wav_write_i16_frames(path, frames, sample_rate):
    """A multichannel WAV: frames[n_frames, n_channels] int16 (1-D: mono), grail_wav_write_i16_frames."""
    frames = np.ascontiguousarray(frames, dtype=np.int16)
    if frames.ndim == 1:
        frames = frames.reshape(-1, 1)
    _check(load().grail_wav_write_i16_frames(path.encode(), frames.ctypes.data, frames.shape[0], frames.shape[1],
                                             int(sample_rate)))


def _mix_items(item_rows, item_offsets, item_tracks, item_gains):
    """The parallel item arrays of the mixing calls (None: all on track 0 / gain 1.0)."""
    rows = np.ascontiguousarray(item_rows, dtype=np.uint32)
    offs = np.ascontiguousarray(item_offsets, dtype=np.uint64)
    tracks, gains = _arr(item_tracks, np.uint32), _arr(item_gains, np.float32)
    assert len(offs) == len(rows) and (tracks is None or len(tracks) == len(rows)) and (gains is None or len(gains) == len(rows))
    return rows, offs, tracks, gains


def mix_place_sequential(row_len, item_rows, item_tracks=None, gaps=None, n_tracks=1):
    """Items laid end to end per track in accumulation order, gaps[i] samples after the previous item on its track
    (grail_mix_place_sequential; pure host).  Returns (item_offsets uint64[n_items], track_len uint64[n_tracks])."""
    row_len = np.ascontiguousarray(row_len, dtype=np.uint32)
    rows = np.ascontiguousarray(item_rows, dtype=np.uint32)
    tracks, gaps = _arr(item_tracks, np.uint32), _arr(gaps, np.int64)
    offs = np.zeros(max(len(rows), 1), dtype=np.uint64)
    track_len = np.zeros(max(n_tracks, 1), dtype=np.uint64)
    _check(load().grail_mix_place_sequential(row_len.ctypes.data, len(row_len), rows.ctypes.data, _ptr(tracks), _ptr(gaps),
                                             len(rows), n_tracks, offs.ctypes.data, track_len.ctypes.data))
    return offs[:len(rows)], track_len[:n_tracks]


def length_bound(segment_lengths, sample_rate):
    """An upper bound of an utterance's length in samples (grail_length_bound); None: no bound."""
    a = np.ascontiguousarray(segment_lengths, dtype=np.float32)
    v = int(load().grail_length_bound(a.ctypes.data_as(C.POINTER(C.c_float)), len(a), float(sample_rate)))
    return None if v == 2 ** 64 - 1 else v


def time_split_warmup(voice):
    """Warm-up length of `voice` for the time-split fast kernels, in samples (0: does not qualify)."""
    return int(load().grail_time_split_warmup(C.byref(voice)))


def fast_sharpness(voice):
    """Predicted bound on |fast - reference| for `voice`, units of 2^-23 (served up to FAST_SHARPNESS_LIMIT)."""
    return float(load().grail_fast_sharpness(C.byref(voice)))


def time_split_grid(span_samples, warmup, chunks, ff_cost_permille=165):
    """Chunk starts of a time-split launch (GrailError when so many chunks do not fit)."""
    out = (C.c_uint32 * max(int(chunks), 1))()
    _check(load().grail_time_split_grid(span_samples, warmup, chunks, ff_cost_permille, out))
    return [int(x) for x in out]


def plan_blocks(rows, span_samples, arithmetic=0, live_formants=4, warmup=3904, compute_units=256):
    """How a batch of `rows` utterances (longest: span_samples) is cut into kernel launches: [PlanBlock]."""
    arr = (PlanBlock * 16)()
    n = C.c_uint32()
    _check(load().grail_plan_blocks(compute_units, arithmetic, live_formants, warmup, rows, span_samples, arr, 16,
                                    C.byref(n)))
    return [PlanBlock.from_buffer_copy(bytes(arr[i])) for i in range(min(n.value, 16))]


def plan_ragged_blocks(row_samples, row_segments=None, row_kinks=None, arithmetic=0, live_formants=4, warmup=3904,
                       compute_units=256):
    """... of a batch whose utterances differ in length: row_samples descending (launch order), the rows' segments and
    kinks of alpha (option "ragged_plan"): [PlanBlock]."""
    rs, sg, kk = (_arr(a, np.uint32) for a in (row_samples, row_segments, row_kinks))
    u32p = C.POINTER(C.c_uint32)
    arr = (PlanBlock * 16)()
    n = C.c_uint32()
    _check(load().grail_plan_ragged_blocks(compute_units, arithmetic, live_formants, warmup, len(rs),
                                           rs.ctypes.data_as(u32p), None if sg is None else sg.ctypes.data_as(u32p),
                                           None if kk is None else kk.ctypes.data_as(u32p), arr, 16, C.byref(n)))
    return [PlanBlock.from_buffer_copy(bytes(arr[i])) for i in range(min(n.value, 16))]


def dispatch_model(workgroup_ms, order=None, compute_units=256, waves_per_workgroup=1):
    """The makespan of workgroups that take workgroup_ms[b], launched in `order`, by the library's model of the workgroup
    dispatcher (grail_dispatch_model; pure host arithmetic)."""
    c = np.ascontiguousarray(workgroup_ms, dtype=np.float64)
    o = _arr(order, np.uint32)
    out = C.c_double()
    _check(load().grail_dispatch_model(compute_units, waves_per_workgroup, c.ctypes.data_as(C.POINTER(C.c_double)),
                                       None if o is None else o.ctypes.data_as(C.POINTER(C.c_uint32)), len(c), C.byref(out)))
    return out.value


def packed_launch_order(workgroup_ms, compute_units=256, waves_per_workgroup=1):
    """order[position] = workgroup: what option "packed_launch_order" launches such workgroups in (grail_packed_launch_order)."""
    c = np.ascontiguousarray(workgroup_ms, dtype=np.float64)
    o = np.zeros(len(c), dtype=np.uint32)
    _check(load().grail_packed_launch_order(compute_units, waves_per_workgroup, c.ctypes.data_as(C.POINTER(C.c_double)), len(c),
                                            o.ctypes.data_as(C.POINTER(C.c_uint32))))
    return o


def device_count():
    n = C.c_int(0)
    st = load().grail_device_count(C.byref(n))
    return n.value if st == OK else 0


def level_gains(mode, item_rows, item_level_db, sumsq=None, peak=None, nonfinite=None, row_len=None, active_level=None,
                n_rows=None):
    """grail_level_gains (pure host): the gain that brings each item's row to item_level_db[i] dB, from the rows' numbers
    (LEVEL_PEAK: peak; LEVEL_RMS: sumsq and row_len; LEVEL_ACTIVE: active_level).  Returns (gains float32[n_items],
    n_unleveled: the items that got gain 0 because their row's level is 0 or it holds a non-finite sample)."""
    sumsq, peak, nonfinite = _arr(sumsq, np.float64), _arr(peak, np.float32), _arr(nonfinite, np.uint32)
    row_len, active_level = _arr(row_len, np.uint32), _arr(active_level, np.float64)
    given = [len(a) for a in (sumsq, peak, nonfinite, row_len, active_level) if a is not None]
    if n_rows is None:
        n_rows = min(given) if given else 0
    assert all(g >= n_rows for g in given)
    rows = np.ascontiguousarray(item_rows, dtype=np.uint32)
    db = np.ascontiguousarray(item_level_db, dtype=np.float32)
    assert len(db) == len(rows)
    gains = np.full(max(len(rows), 1), np.nan, dtype=np.float32)
    n_unleveled = C.c_uint32(0xFFFFFFFF)
    _check(load().grail_level_gains(int(mode), _ptr(sumsq), _ptr(peak), _ptr(nonfinite), _ptr(row_len), _ptr(active_level),
                                    n_rows, rows.ctypes.data, db.ctypes.data, len(rows), gains.ctypes.data,
                                    C.addressof(n_unleveled)))
    return gains[:len(rows)], n_unleveled.value


def active_level(frame_sumsq, row_len, frame=LEVEL_FRAME, floor_db=LEVEL_ACTIVE_FLOOR_DB):
    """grail_active_level (pure host): sqrt(mean square) over the frames within floor_db of the loudest frame."""
    fs = np.ascontiguousarray(frame_sumsq, dtype=np.float64)
    assert len(fs) >= -(-int(row_len) // int(frame))
    return float(load().grail_active_level(fs.ctypes.data, int(row_len), int(frame), float(floor_db)))


def kweighting(sample_rate):
    """grail_kweighting (pure host): the ten K-weighting coefficients for a sample rate, float64[10]: b0 b1 b2 a1 a2 of the
    shelf, then of the high-pass."""
    coef = np.full(10, np.nan, dtype=np.float64)
    _check(load().grail_kweighting(int(sample_rate), coef.ctypes.data))
    return coef


def gated_mean_square(hop_sumsq, hop):
    """grail_gated_mean_square (pure host): the BS.1770 gate over one row's hop sums; hop = sample_rate // 10."""
    hs = np.ascontiguousarray(hop_sumsq, dtype=np.float64)
    return float(load().grail_gated_mean_square(hs.ctypes.data if len(hs) else None, len(hs), int(hop)))


def loudness_lufs(gated_ms):
    """grail_loudness_lufs: -0.691 + 10 log10(gated mean square); -inf for 0."""
    return float(load().grail_loudness_lufs(float(gated_ms)))


def loudness_level(gated_ms):
    """grail_loudness_level: the level whose 20 log10 is the loudness in LUFS."""
    return float(load().grail_loudness_level(float(gated_ms)))


def loudness_window_max(hop_sumsq, hop, window_hops):
    """grail_loudness_window_max (pure host): the largest mean square over windows of window_hops hops, one every hop:
    4 = momentary, 30 = short-term; loudness_lufs() gives its LUFS.  0 for fewer hops than the window."""
    hs = np.ascontiguousarray(hop_sumsq, dtype=np.float64)
    return float(load().grail_loudness_window_max(hs.ctypes.data if len(hs) else None, len(hs), int(hop), int(window_hops)))


def loudness_range(hop_sumsq, hop):
    """grail_loudness_range (pure host): the loudness range in LU (EBU Tech 3342) of one row's hop sums; 0 for fewer than
    30 hops or nothing above the absolute gate."""
    hs = np.ascontiguousarray(hop_sumsq, dtype=np.float64)
    return float(load().grail_loudness_range(hs.ctypes.data if len(hs) else None, len(hs), int(hop)))


def true_peak_coefficients():
    """grail_true_peak_coefficients (pure host): the 4 x 12 taps of the BS.1770-4 Annex 2 filter, float64[4, 12]."""
    coef = np.full((TRUE_PEAK_PHASES, TRUE_PEAK_TAPS), np.nan, dtype=np.float64)
    _check(load().grail_true_peak_coefficients(coef.ctypes.data))
    return coef


def true_peak_db(true_peak):
    """grail_true_peak_db: 20 log10(true peak) in dBTP; -inf for 0."""
    return float(load().grail_true_peak_db(float(true_peak)))


def limit_ceiling(ceiling_db):
    """grail_limit_ceiling (pure host): the float32 that a ceiling in dBTP is to grail_limit_async."""
    return np.float32(load().grail_limit_ceiling(float(np.float32(ceiling_db))))


def _out_u64(fn, *args):
    """the uint64 a `*_len` / `*_hops` function writes behind its last argument"""
    out = C.c_uint64(0)
    _check(fn(*args, C.addressof(out)))
    return out.value


def limit_stream_len(fed_before, n, lookahead_log2, finishing=False):
    """grail_limit_stream_len (pure host): the outputs a call on a limit stream writes for a group that was fed fed_before
    samples before it: a `next` call that feeds n samples, or (finishing, n = 0) the tail of `finish`."""
    return _out_u64(load().grail_limit_stream_len, fed_before, n, lookahead_log2, 1 if finishing else 0)


def resample_ratio(rate_in, rate_out):
    """grail_resample_ratio (pure host): (up, down, taps) of a pair of whole-numbered rates; GrailError for a pair that is
    not supported (a rate of 0, equal rates, more than RESAMPLE_TABLE_MAX table entries)."""
    u, d, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _check(load().grail_resample_ratio(rate_in, rate_out, C.addressof(u), C.addressof(d), C.addressof(p)))
    return u.value, d.value, p.value


def resample_coefficients(rate_in, rate_out):
    """grail_resample_coefficients (pure host): the numerators N of 2^26 of the pair's table, int32[up, taps]."""
    u, _, p = resample_ratio(rate_in, rate_out)
    num = np.zeros((u, p), dtype=np.int32)
    _check(load().grail_resample_coefficients(rate_in, rate_out, num.ctypes.data, u * p))
    return num


def resample_len(n, rate_in, rate_out):
    """grail_resample_len (pure host): ceil(n * up / down), the length of a row of n samples resampled."""
    return _out_u64(load().grail_resample_len, n, rate_in, rate_out)


def resample_stream_len(fed_before, n, rate_in, rate_out, finishing=False):
    """grail_resample_stream_len (pure host): the outputs a call on a resample stream writes for a row that was fed
    fed_before samples before it: a `next` call that feeds n samples, or (finishing, n = 0) the tail of `finish`."""
    return _out_u64(load().grail_resample_stream_len, fed_before, n, rate_in, rate_out, 1 if finishing else 0)


def fir_len(n, n_taps, origin):
    """grail_fir_len (pure host): 0 for n = 0, else n + n_taps - 1 - origin, the length of a row of n samples filtered."""
    return _out_u64(load().grail_fir_len, n, n_taps, origin)


def fir_stream_len(fed_before, n, n_taps, origin, finishing=False):
    """grail_filter_stream_len (pure host): the outputs a call on a filter stream writes for a row that was fed fed_before
    samples before it: a `next` call that feeds n samples, or (finishing, n = 0) the tail of `finish`."""
    return _out_u64(load().grail_filter_stream_len, fed_before, n, n_taps, origin, 1 if finishing else 0)


def fir_design(sample_rate, lo_hz, hi_hz, n_taps):
    """grail_fir_design (pure host): float32[n_taps] of the Kaiser-windowed band-pass lo_hz .. hi_hz at sample_rate (n_taps
    odd; lo_hz = 0: a low-pass, hi_hz = sample_rate / 2: a high-pass).  The origin to use is (n_taps - 1) // 2."""
    taps = np.zeros(max(int(n_taps), 1), dtype=np.float32)
    _check(load().grail_fir_design(sample_rate, lo_hz, hi_hz, n_taps, taps.ctypes.data))
    return taps


def iir_design(kind, sample_rate, f0_hz, q, gain_db=0.0):
    """grail_iir_design (pure host): float64[5] = b0 b1 b2 a1 a2 of one biquad section of `kind` (IIR_LOWPASS ... IIR_HIGHSHELF)
    at f0_hz with quality q; gain_db is read by the shelves and the peak."""
    coef = np.zeros(5, dtype=np.float64)
    _check(load().grail_iir_design(kind, sample_rate, f0_hz, q, gain_db, coef.ctypes.data))
    return coef


def iir_block_matrix(coef):
    """grail_biquad_block_matrix (pure host): float64 [2 S][2 S], the block transition matrix of one filter (float64 [S][5] or
    flat [5 S]): state i (s1[0] s2[0] s1[1] ...) after IIR_BLOCK steps on +0.0 from the unit state c, at [i][c]."""
    flat = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
    assert len(flat) % 5 == 0
    S = len(flat) // 5
    matrix = np.zeros((2 * S, 2 * S), dtype=np.float64)
    _check(load().grail_biquad_block_matrix(flat.ctypes.data, S, matrix.ctypes.data))
    return matrix


def iir_stream_len(fed_before, n, tail, finishing=False):
    """grail_iir_stream_len (pure host): the outputs a call on an IIR stream writes for a row that was fed fed_before samples
    before it: n for a `next` call that feeds n; for `finish` (n must be 0) the tail, or 0 for a row that was fed nothing."""
    return _out_u64(load().grail_iir_stream_len, fed_before, n, tail, 1 if finishing else 0)


def dyn_design(kind, detector, threshold_db, ratio, knee_db=0.0, range_db=0.0, makeup_db=0.0):
    """grail_dyn_design (pure host): float64[DYN_POINTS], the gain curve of a compressor (DYN_COMPRESS) or a downward expander
    (DYN_EXPAND; range_db: the most it takes away) over the levels of the detector's envelope (DYN_PEAK or DYN_SQUARE)."""
    gain = np.zeros(DYN_POINTS, dtype=np.float64)
    _check(load().grail_dyn_design(kind, detector, threshold_db, ratio, knee_db, range_db, makeup_db, gain.ctypes.data))
    return gain


def dyn_ballistics(sample_rate, attack_ms, release_ms):
    """grail_dyn_ballistics (pure host): float64[2] = alpha_attack, alpha_release of an envelope that covers 1 - 1/e of a step
    in attack_ms on the way up and release_ms on the way down; 0.0 for a time of 0."""
    alpha = np.zeros(2, dtype=np.float64)
    _check(load().grail_dyn_ballistics(sample_rate, attack_ms, release_ms, alpha.ctypes.data))
    return alpha


def true_peak_limit_gains(true_peak, item_rows, item_gains, ceiling_db, n_rows=None):
    """grail_true_peak_limit_gains (pure host): the gains capped so that |gain| * true_peak[row] <= 10^(ceiling_db / 20).
    Returns (gains float32[n_items], a copy; n_limited: the items that were changed)."""
    tp = np.ascontiguousarray(true_peak, dtype=np.float64)
    rows = np.ascontiguousarray(item_rows, dtype=np.uint32)
    gains = np.array(item_gains, dtype=np.float32, ndmin=1)
    assert len(gains) == len(rows)
    n_limited = C.c_uint32(0xFFFFFFFF)
    _check(load().grail_true_peak_limit_gains(tp.ctypes.data, len(tp) if n_rows is None else n_rows, rows.ctypes.data,
                                              len(rows), float(ceiling_db), gains.ctypes.data, C.addressof(n_limited)))
    return gains, n_limited.value


def meter_stream_hops(fed_before, n, sample_rate):
    """grail_meter_stream_hops (pure host): the hops a `next` call on a meter stream completes for a row that was fed fed_before
    samples before it and is fed n: (fed_before + n) // H - fed_before // H, H = sample_rate // 10."""
    return _out_u64(load().grail_meter_stream_hops, fed_before, n, sample_rate)
