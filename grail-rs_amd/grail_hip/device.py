"""What runs on a device: Context (one per process and GPU), its batches and streams, Node (one process, several GPUs),
and the one waited-for form behind every call that returns results the device computed."""
import ctypes as C

import numpy as np

from ._abi import (DYN_POINTS, ERR_BUFFER_TOO_SMALL, LEVEL_RMS, MIX_ACCUMULATE, OUT_HOST, PHONEME_DTYPE, UNIQUE_ID_BYTES,
                   SequenceElem, Voice, _arr, _check, _ptr, limit_stream_delay, load)
from .host import _mix_items


class Batch:
    def __init__(self, ctx, handle, n_utt):
        self.ctx, self.handle, self.n_utt = ctx, handle, n_utt

    def lengths(self, max_len=0xFFFFFFFF):
        out = np.zeros(max(self.n_utt, 1), dtype=np.uint32)
        _check(load().grail_batch_lengths(self.ctx.handle, self.handle, max_len, out.ctypes.data))
        return out[: self.n_utt]

    def synthesize_async(self, out_dev, out_stride, out_len_dev=None):
        _check(load().grail_batch_synthesize_async(self.ctx.handle, self.handle, out_dev,
                                                   out_stride, out_len_dev))

    def synthesize_pcm16_async(self, out_dev, out_stride, out_len_dev=None):
        """Rows of i16 PCM: the WAV sink's conversion fused into the kernel's store."""
        _check(load().grail_batch_synthesize_pcm16_async(self.ctx.handle, self.handle, out_dev,
                                                         out_stride, out_len_dev))

    def mix(self, item_rows, item_offsets, tracks_dev, track_stride, n_tracks, track_len, item_tracks=None,
            item_gains=None, accumulate=False):
        """grail_batch_mix: the batch rendered in blocks of rows and mixed into tracks_dev [n_tracks][track_stride]
        (synchronous).  Returns the rows' lengths."""
        rows, offs, tracks, gains = _mix_items(item_rows, item_offsets, item_tracks, item_gains)
        out_len = np.zeros(max(self.n_utt, 1), dtype=np.uint32)
        _check(load().grail_batch_mix(self.ctx.handle, self.handle, rows.ctypes.data, _ptr(tracks), offs.ctypes.data,
                                      _ptr(gains), len(rows), tracks_dev, track_stride, n_tracks, track_len,
                                      out_len.ctypes.data, MIX_ACCUMULATE if accumulate else 0))
        return out_len[:self.n_utt]

    def mix_leveled(self, item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len,
                    item_tracks=None, mode=LEVEL_RMS, accumulate=False):
        """grail_batch_mix_leveled: mix() with a level in dB per item instead of a gain; every block's rows are measured on
        the device between rendering and mixing.  Returns (the rows' lengths, the gains used, n_unleveled)."""
        return self._mix_leveled(item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len,
                                 item_tracks, mode, accumulate, None)[:3]

    def mix_leveled_limited(self, item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len,
                            ceiling_db, item_tracks=None, mode=LEVEL_RMS, accumulate=False):
        """grail_batch_mix_leveled_limited: mix_leveled() under a true-peak ceiling in dBTP; the rows' true peaks are
        measured too and cap the gains.  Returns (the rows' lengths, the gains used, n_unleveled, n_limited)."""
        return self._mix_leveled(item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len,
                                 item_tracks, mode, accumulate, float(ceiling_db))

    def _mix_leveled(self, item_rows, item_offsets, item_level_db, tracks_dev, track_stride, n_tracks, track_len, item_tracks,
                     mode, accumulate, ceiling_db):
        rows, offs, tracks, _ = _mix_items(item_rows, item_offsets, item_tracks, None)
        db = np.ascontiguousarray(item_level_db, dtype=np.float32)
        assert len(db) == len(rows)
        out_len = np.zeros(max(self.n_utt, 1), dtype=np.uint32)
        gains = np.zeros(max(len(rows), 1), dtype=np.float32)
        n_unleveled, n_limited = C.c_uint32(0), C.c_uint32(0)
        flags = MIX_ACCUMULATE if accumulate else 0
        if ceiling_db is None:
            _check(load().grail_batch_mix_leveled(self.ctx.handle, self.handle, rows.ctypes.data, _ptr(tracks), offs.ctypes.data,
                                                  db.ctypes.data, int(mode), len(rows), tracks_dev, track_stride, n_tracks,
                                                  track_len, out_len.ctypes.data, gains.ctypes.data, C.addressof(n_unleveled),
                                                  flags))
        else:
            _check(load().grail_batch_mix_leveled_limited(
                self.ctx.handle, self.handle, rows.ctypes.data, _ptr(tracks), offs.ctypes.data, db.ctypes.data, int(mode),
                len(rows), tracks_dev, track_stride, n_tracks, track_len, out_len.ctypes.data, gains.ctypes.data,
                C.addressof(n_unleveled), ceiling_db, C.addressof(n_limited), flags))
        return out_len[:self.n_utt], gains[:len(rows)], n_unleveled.value, n_limited.value

    def free(self):
        if self.handle:
            load().grail_batch_free(self.ctx.handle, self.handle)
            self.handle = None


def _marks(which, n):
    """the `which` of a finishing call (a host sequence of n, non-zero = marked; None: all of them) as bytes"""
    marks = _arr(which, np.uint8)
    assert marks is None or len(marks) == n
    return marks


def _coef10(coef):
    """the optional ten K-weighting coefficients of a call (None: the library's own for the sample rate)"""
    c = _arr(coef, np.float64)
    assert c is None or c.shape == (10,)
    return c


class Stream:
    """grail_stream: resumable synthesis of a Batch (chunks of samples per call)."""

    def __init__(self, batch):
        self.batch, self.ctx = batch, batch.ctx
        h = C.c_void_p()
        _check(load().grail_stream_open(self.ctx.handle, batch.handle, C.byref(h)))
        self.handle = h

    def next_async(self, max_samples, out_dev, out_stride, out_len_dev=None):
        _check(load().grail_stream_next_async(self.ctx.handle, self.handle, max_samples, out_dev,
                                              out_stride, out_len_dev))

    def next_pcm16_async(self, max_samples, out_dev, out_stride, out_len_dev=None):
        _check(load().grail_stream_next_pcm16_async(self.ctx.handle, self.handle, max_samples,
                                                    out_dev, out_stride, out_len_dev))

    def close(self):
        if self.handle:
            load().grail_stream_close(self.ctx.handle, self.handle)
            self.handle = None


class LiveStream(Stream):
    """grail_stream_open_live: n_utt chains whose sources deliver while they run (examples/interactive.rs:31-48)."""

    def __init__(self, ctx, n_utt, voice_ids=None, jitter_seeds=None, ring_segments=0, elems=False):
        self.ctx, self.n_utt, self.elems, self.batch = ctx, n_utt, elems, None
        voice_ids, jitter_seeds = _arr(voice_ids, np.uint32), _arr(jitter_seeds, np.uint32)
        assert (voice_ids is None or len(voice_ids) == n_utt) and (jitter_seeds is None or len(jitter_seeds) == n_utt)
        h = C.c_void_p()
        _check(load().grail_stream_open_live(ctx.handle, n_utt, _ptr(voice_ids), _ptr(jitter_seeds), ring_segments,
                                             1 if elems else 0, C.byref(h)))
        self.handle = h

    def append(self, segs, seg_offsets):
        """Utterance u receives segs[seg_offsets[u]:seg_offsets[u + 1]] behind what it already has."""
        seg_offsets = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
        assert len(seg_offsets) == self.n_utt + 1
        if self.elems:
            arr = (SequenceElem * max(len(segs), 1))(*segs)
            _check(load().grail_stream_append_elems(self.ctx.handle, self.handle, C.cast(arr, C.c_void_p),
                                                    seg_offsets.ctypes.data))
        else:
            segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
            _check(load().grail_stream_append(self.ctx.handle, self.handle, segs.ctypes.data, seg_offsets.ctypes.data))

    def finish(self, which=None):
        marks = _marks(which, self.n_utt)
        _check(load().grail_stream_finish(self.ctx.handle, self.handle, _ptr(marks)))

    def pending(self):
        out = np.zeros(self.n_utt, dtype=np.uint32)
        _check(load().grail_stream_pending(self.ctx.handle, self.handle, out.ctypes.data))
        return out


def _waited(ctx, specs, call):
    """The waited-for form of a call whose results are device arrays.  specs: per result (shape, dtype) or (shape, dtype,
    fill), or None for a result that is not wanted.  Every result gets a device array (never of zero bytes; None for
    None); those with a fill are uploaded holding it first, for the calls that leave entries past a row's end unwritten;
    call(*device_arrays) runs; the results are copied back; the wait and the release whatever happened.  Returns a tuple,
    an array of exactly that shape (or None) per spec."""
    res = [None if s is None else np.full(s[0], s[2] if len(s) > 2 else 0, dtype=s[1]) for s in specs]
    dev = []
    try:
        for r in res:
            dev.append(None if r is None else ctx.device_alloc(max(r.nbytes, 8)))
        for r, d, s in zip(res, dev, specs):
            if r is not None and len(s) > 2 and r.nbytes:
                ctx.h2d(d, r, r.nbytes)
        call(*dev)
        for r, d in zip(res, dev):
            if r is not None and r.nbytes:
                ctx.d2h(r, d, r.nbytes)
    finally:
        ctx.sync()
        for d in dev:
            if d is not None:
                ctx.device_free(d)
    return tuple(res)


def _per(n, *dtypes):
    """the specs of results that are n words each, one per row or group"""
    return [((n,), t) for t in dtypes]


class LimitStream:
    """A limit stream of a Context (Context.limit_stream_open), beside the fir_stream_* and resample_stream_* helpers: the
    handle with what the waited-for forms need to size their results, one per group."""

    def __init__(self, ctx, handle, n_rows, group, lookahead_log2):
        self.ctx, self.handle, self.n_rows, self.group, self.lookahead_log2 = ctx, handle, n_rows, group, lookahead_log2
        self.n_groups = n_rows // group
        self.delay = limit_stream_delay(lookahead_log2)

    def next_async(self, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None, min_gain_dev=None,
                   n_limited_dev=None, nonfinite_dev=None):
        """grail_limit_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples; the outputs that
        became known go to out_dev + u * out_stride.  Results are DEVICE arrays [n_groups] (any may be None), queued on the
        context's stream; in_dev may be reused by what is queued behind the call."""
        _check(load().grail_limit_stream_next_async(self.ctx.handle, self.handle, in_dev, in_stride, in_len_dev, out_dev, out_stride,
                                                    out_len_dev, min_gain_dev, n_limited_dev, nonfinite_dev))

    def next(self, in_dev, in_stride, in_len_dev, out_dev, out_stride):
        """next_async, waited for, the results copied back: (out_len uint32, min_gain float32, n_limited uint32, nonfinite
        uint32), one per group; a refused group reads (LIMIT_REFUSED, NaN, 0, 0)."""
        return _waited(self.ctx, _per(self.n_groups, np.uint32, np.float32, np.uint32, np.uint32),
                       lambda *d: self.next_async(in_dev, in_stride, in_len_dev, out_dev, out_stride, *d))

    def finish_async(self, out_dev, out_stride, which=None, out_len_dev=None, min_gain_dev=None, n_limited_dev=None):
        """grail_limit_stream_finish_async: the groups marked in which (a host sequence, non-zero = marked; None: every group)
        that have not ended write their tails (at most `delay` samples a row) and end."""
        marks = _marks(which, self.n_groups)
        _check(load().grail_limit_stream_finish_async(self.ctx.handle, self.handle, _ptr(marks), out_dev, out_stride, out_len_dev,
                                                      min_gain_dev, n_limited_dev))

    def finish(self, out_dev, out_stride, which=None):
        """finish_async, waited for: (out_len uint32, min_gain float32, n_limited uint32), one per group; (0, 1.0, 0) for
        groups not marked or ended before."""
        return _waited(self.ctx, _per(self.n_groups, np.uint32, np.float32, np.uint32),
                       lambda *d: self.finish_async(out_dev, out_stride, which, *d))

    def close(self):
        """grail_limit_stream_close: waits for the context's stream, then releases the stream."""
        if self.handle is not None:
            _check(load().grail_limit_stream_close(self.ctx.handle, self.handle))
            self.handle = None


class MeterStream:
    """A meter stream of a Context (Context.meter_stream_open), in the style of LimitStream: the handle with what the waited-for
    forms need to size their results, one per row."""

    def __init__(self, ctx, handle, n_rows, sample_rate, max_hops):
        self.ctx, self.handle, self.n_rows, self.sample_rate, self.max_hops = ctx, handle, n_rows, sample_rate, max_hops
        self.hop = sample_rate // 10

    def hops_stride(self, in_stride):
        """the least hops_stride of a call that feeds rows of in_stride: the most hops a row can complete in it"""
        return (in_stride + self.hop - 1) // self.hop

    def next_async(self, in_dev, in_stride, in_len_dev, hop_sumsq_dev=None, hops_stride=0, n_hops_dev=None, true_peak_dev=None,
                   nonfinite_dev=None):
        """grail_meter_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples; the hops the call
        completes go to hop_sumsq_dev + u * hops_stride (float64).  Results are DEVICE arrays [n_rows] (uint32, float64,
        uint32; any may be None), queued on the context's stream; in_dev may be reused by what is queued behind the call."""
        _check(load().grail_meter_stream_next_async(self.ctx.handle, self.handle, in_dev, in_stride, in_len_dev, hop_sumsq_dev,
                                                    hops_stride, n_hops_dev, true_peak_dev, nonfinite_dev))

    def next(self, in_dev, in_stride, in_len_dev, hop_sumsq_dev=None, hops_stride=0):
        """next_async, waited for, the results copied back: (n_hops uint32, true_peak float64, nonfinite uint32), one per
        row; a refused row reads (LIMIT_REFUSED, NaN, 0)."""
        return _waited(self.ctx, _per(self.n_rows, np.uint32, np.float64, np.uint32),
                       lambda *d: self.next_async(in_dev, in_stride, in_len_dev, hop_sumsq_dev, hops_stride, *d))

    def read_async(self, integrated_ms_dev=None, momentary_ms_dev=None, short_term_ms_dev=None, true_peak_dev=None, hops_dev=None):
        """grail_meter_stream_read_async: what the meter shows of every row now, DEVICE arrays [n_rows] of float64 (hops_dev:
        uint64), any may be None; changes no state."""
        _check(load().grail_meter_stream_read_async(self.ctx.handle, self.handle, integrated_ms_dev, momentary_ms_dev,
                                                    short_term_ms_dev, true_peak_dev, hops_dev))

    def read(self):
        """read_async, waited for: (integrated_ms, momentary_ms, short_term_ms, true_peak float64, hops uint64), one per row."""
        return _waited(self.ctx, _per(self.n_rows, np.float64, np.float64, np.float64, np.float64, np.uint64), self.read_async)

    def ledger(self):
        """grail_meter_stream_ledger: (the ledger's device address, its stride in float64); row u's hop sums lie at
        address + 8 * (u * stride + h), h below the row's hops."""
        base, stride = C.c_void_p(), C.c_uint64()
        _check(load().grail_meter_stream_ledger(self.ctx.handle, self.handle, C.addressof(base), C.addressof(stride)))
        return base, stride.value

    def ledger_rows(self):
        """the rows' hop sums so far, copied from the ledger: a list of float64 arrays, one per row"""
        hops = self.read()[4]
        base, stride = self.ledger()
        rows = []
        for u, h in enumerate(hops):
            row = np.zeros(int(h), dtype=np.float64)
            if h:
                self.ctx.d2h(row, C.c_void_p(base.value + 8 * u * stride), row.nbytes)
            rows.append(row)
        return rows

    def finish_async(self, which=None, true_peak_dev=None):
        """grail_meter_stream_finish_async: the rows marked in which (a host sequence, non-zero = marked; None: every row) that
        have not ended ring out over the eleven outputs after their last sample and end."""
        marks = _marks(which, self.n_rows)
        _check(load().grail_meter_stream_finish_async(self.ctx.handle, self.handle, _ptr(marks), true_peak_dev))

    def finish(self, which=None):
        """finish_async, waited for: the largest of each row's eleven last outputs, float64; +0.0 for rows not marked or ended
        before."""
        return _waited(self.ctx, _per(self.n_rows, np.float64), lambda d: self.finish_async(which, d))[0]

    def close(self):
        """grail_meter_stream_close: waits for the context's stream, then releases the stream."""
        if self.handle is not None:
            _check(load().grail_meter_stream_close(self.ctx.handle, self.handle))
            self.handle = None


class Context:
    """grail_ctx: one per (process, GPU)."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(load().grail_create(device, C.byref(h)))
        self.handle = h
        self.device = device

    def close(self):
        if self.handle:
            load().grail_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_voices(self, voices):
        arr = (Voice * len(voices))(*[v.copy() for v in voices])
        _check(load().grail_set_voices(self.handle, C.cast(arr, C.c_void_p), len(voices)))

    def get_voices(self):
        n = C.c_uint32()
        _check(load().grail_get_voices(self.handle, None, 0, C.byref(n)))
        arr = (Voice * max(n.value, 1))()
        _check(load().grail_get_voices(self.handle, C.cast(arr, C.c_void_p), n.value, C.byref(n)))
        return [arr[i].copy() for i in range(n.value)]

    def pci_bus_id(self):
        buf = C.create_string_buffer(32)
        _check(load().grail_device_pci_bus_id(self.handle, buf, 32))
        return buf.value.decode()

    def set_option(self, name, value):
        _check(load().grail_set_option(self.handle, name.encode(), value))

    def get_option(self, name):
        v = C.c_int64()
        _check(load().grail_get_option(self.handle, name.encode(), C.byref(v)))
        return v.value

    @staticmethod
    def _prep(segs_dtype, segs, seg_offsets, voice_ids, jitter_seeds):
        seg_offsets = np.ascontiguousarray(seg_offsets, dtype=np.uint32)
        n_utt = len(seg_offsets) - 1
        voice_ids, jitter_seeds = _arr(voice_ids, np.uint32), _arr(jitter_seeds, np.uint32)
        assert (voice_ids is None or len(voice_ids) == n_utt) and (jitter_seeds is None or len(jitter_seeds) == n_utt)
        return seg_offsets, n_utt, voice_ids, jitter_seeds

    def upload(self, segs, seg_offsets, voice_ids=None, jitter_seeds=None):
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, segs, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        h = C.c_void_p()
        _check(load().grail_batch_upload(self.handle, segs.ctypes.data, seg_offsets.ctypes.data,
                                         _ptr(voice_ids), _ptr(jitter_seeds), n_utt, C.byref(h)))
        return Batch(self, h, n_utt)

    def upload_elems(self, seq_elems, seg_offsets, voice_ids=None, jitter_seeds=None):
        arr = (SequenceElem * max(len(seq_elems), 1))(*seq_elems)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, None, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        h = C.c_void_p()
        _check(load().grail_batch_upload_elems(self.handle, C.cast(arr, C.c_void_p),
                                               seg_offsets.ctypes.data, _ptr(voice_ids),
                                               _ptr(jitter_seeds), n_utt, C.byref(h)))
        return Batch(self, h, n_utt)

    def synthesize(self, segs, seg_offsets, voice_ids=None, jitter_seeds=None, out_stride=None,
                   allow_truncation=False):
        """One-call form over host buffers.  Returns (out[n_utt, out_stride], out_len)."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, segs, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        if out_stride is None:
            b = self.upload(segs, seg_offsets, voice_ids, jitter_seeds)
            try:
                lens = b.lengths()
            finally:
                b.free()
            out_stride = int((max(int(lens.max()) if n_utt else 0, 1) + 3) // 4 * 4)
        out = np.zeros((max(n_utt, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        st = load().grail_synthesize_batch(self.handle, segs.ctypes.data, seg_offsets.ctypes.data,
                                           _ptr(voice_ids), _ptr(jitter_seeds), n_utt,
                                           out.ctypes.data, out_stride, out_len.ctypes.data,
                                           OUT_HOST)
        if not (allow_truncation and st == ERR_BUFFER_TOO_SMALL):
            _check(st)
        return out[:n_utt], out_len[:n_utt]

    def synthesize_pcm16(self, segs, seg_offsets, voice_ids=None, jitter_seeds=None, out_stride=4096):
        """One-call form with i16 PCM rows (examples/cli.rs:49 on the device)."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, segs, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        out = np.zeros((max(n_utt, 1), out_stride), dtype=np.int16)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_synthesize_batch_pcm16(
            self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids),
            _ptr(jitter_seeds), n_utt, out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n_utt], out_len[:n_utt]

    def synthesize_elems(self, seq_elems, seg_offsets, voice_ids=None, jitter_seeds=None,
                         out_stride=4096):
        arr = (SequenceElem * max(len(seq_elems), 1))(*seq_elems)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, None, seg_offsets,
                                                                 voice_ids, jitter_seeds)
        out = np.zeros((max(n_utt, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_synthesize_batch_elems(
            self.handle, C.cast(arr, C.c_void_p), seg_offsets.ctypes.data, _ptr(voice_ids),
            _ptr(jitter_seeds), n_utt, out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n_utt], out_len[:n_utt]

    def say(self, texts, voice_ids=None, jitter_seeds=None, out_stride=None, seconds_per_char=1.6):
        """examples/cli.rs:175-184 for a list of texts. Returns (out[n, stride], out_len)."""
        n = len(texts)
        arr = (C.c_char_p * max(n, 1))(*[t.encode("utf-8") for t in texts])
        voice_ids, jitter_seeds = _arr(voice_ids, np.uint32), _arr(jitter_seeds, np.uint32)
        if out_stride is None:
            rate = max(v.sample_rate for v in self.get_voices())
            longest = max([len(t) for t in texts] + [1])
            out_stride = (int((longest * seconds_per_char + 1.0) * rate) + 63) // 64 * 64
        out = np.zeros((max(n, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n, 1), dtype=np.uint32)
        _check(load().grail_say_batch(self.handle, arr, n, _ptr(voice_ids), _ptr(jitter_seeds),
                                      out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n], out_len[:n]

    def pcm16(self, in_dev, in_stride, len_dev, n_utt, max_len, out_dev, out_stride):
        _check(load().grail_pcm16_async(self.handle, in_dev, in_stride, len_dev, n_utt, max_len,
                                        out_dev, out_stride))

    def mix_async(self, rows_dev, row_stride, row_len, item_rows, item_offsets, tracks_dev, track_stride, n_tracks,
                  track_len, item_tracks=None, item_gains=None, accumulate=False):
        """grail_mix_async: rows_dev [n_rows][row_stride] (row_len: host, one per row) mixed into tracks_dev
        [n_tracks][track_stride], queued on the context's stream."""
        row_len = np.ascontiguousarray(row_len, dtype=np.uint32)
        rows, offs, tracks, gains = _mix_items(item_rows, item_offsets, item_tracks, item_gains)
        _check(load().grail_mix_async(self.handle, rows_dev, row_stride, row_len.ctypes.data, len(row_len),
                                      rows.ctypes.data, _ptr(tracks), offs.ctypes.data, _ptr(gains), len(rows),
                                      tracks_dev, track_stride, n_tracks, track_len,
                                      MIX_ACCUMULATE if accumulate else 0))

    def pcm16_frames_async(self, tracks_dev, track_stride, n_tracks, n_frames, frames_dev):
        """grail_pcm16_frames_async: tracks -> interleaved i16 frames (frames_dev[f * n_tracks + t])."""
        _check(load().grail_pcm16_frames_async(self.handle, tracks_dev, track_stride, n_tracks, n_frames, frames_dev))

    def levels_async(self, rows_dev, row_stride, len_dev, n_rows, sumsq_dev=None, peak_dev=None, nonfinite_dev=None):
        """grail_levels_async: per row the binary64 sum of squares, the largest finite |x| and the count of non-finite
        samples, into DEVICE arrays [n_rows] (any may be None), queued on the context's stream."""
        _check(load().grail_levels_async(self.handle, rows_dev, row_stride, len_dev, n_rows, sumsq_dev, peak_dev,
                                         nonfinite_dev))

    def levels(self, rows_dev, row_stride, len_dev, n_rows):
        """levels_async, waited for and copied back: (sumsq float64, peak float32, nonfinite uint32), one per row."""
        return _waited(self, _per(n_rows, np.float64, np.float32, np.uint32),
                       lambda *d: self.levels_async(rows_dev, row_stride, len_dev, n_rows, *d))

    def frame_levels_async(self, rows_dev, row_stride, len_dev, n_rows, frame, frame_sumsq_dev, frame_peak_dev,
                           frames_stride):
        """grail_frame_levels_async: per frame of `frame` samples, into DEVICE arrays [n_rows][frames_stride]."""
        _check(load().grail_frame_levels_async(self.handle, rows_dev, row_stride, len_dev, n_rows, frame, frame_sumsq_dev,
                                               frame_peak_dev, frames_stride))

    def frame_levels(self, rows_dev, row_stride, len_dev, n_rows, frame, fill=None):
        """frame_levels_async, waited for and copied back: (sumsq float64 [n_rows, frames], peak float32 [n_rows, frames])
        with frames = ceil(row_stride / frame).  Frames past a row's end hold `fill` (default NaN): the call leaves them
        unwritten."""
        frames = max(-(-int(row_stride) // int(frame)), 1)
        fill = np.nan if fill is None else fill
        return _waited(self, [((n_rows, frames), np.float64, fill), ((n_rows, frames), np.float32, fill)],
                       lambda s, p: self.frame_levels_async(rows_dev, row_stride, len_dev, n_rows, frame, s, p, frames))

    def loudness_async(self, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef=None, gated_ms_dev=None,
                       hop_sumsq_dev=None, hops_stride=0, nonfinite_dev=None):
        """grail_loudness_async: per row the K-weighted gated mean square, the hop sums [n_rows][hops_stride] and the count
        of non-finite samples, into DEVICE arrays (any may be None), queued on the context's stream.  coef: ten float64 or
        None = kweighting(sample_rate)."""
        c = _coef10(coef)
        _check(load().grail_loudness_async(self.handle, rows_dev, row_stride, len_dev, n_rows, int(sample_rate), _ptr(c),
                                           gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev))

    def loudness_segmented_async(self, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef=None, gated_ms_dev=None,
                                 hop_sumsq_dev=None, hops_stride=0, nonfinite_dev=None):
        """grail_loudness_segmented_async: loudness_async's arguments and outputs, every hop filtered from a zero state
        LOUDNESS_WARMUP_HOPS hops before it, one lane per hop: for few long rows (a finished track)."""
        c = _coef10(coef)
        _check(load().grail_loudness_segmented_async(self.handle, rows_dev, row_stride, len_dev, n_rows, int(sample_rate),
                                                     _ptr(c), gated_ms_dev, hop_sumsq_dev, hops_stride, nonfinite_dev))

    def loudness_segmented(self, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef=None, hops=True, fill=None):
        """loudness_segmented_async, waited for and copied back: what loudness() returns."""
        return self._loudness_sync(self.loudness_segmented_async, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, hops,
                                   fill)

    def loudness(self, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef=None, hops=True, fill=None):
        """loudness_async, waited for and copied back: (gated_ms float64 [n_rows], hop_sumsq float64 [n_rows, row_stride //
        hop] or None, nonfinite uint32 [n_rows]).  Hops past a row's last hold `fill` (default NaN): the call leaves them
        unwritten."""
        return self._loudness_sync(self.loudness_async, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, hops, fill)

    def _loudness_sync(self, call, rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, hops, fill):
        hop = int(sample_rate) // 10
        hs = max(int(row_stride) // hop, 1) if hop else 1
        hop_sums = ((n_rows, hs), np.float64, np.nan if fill is None else fill) if hops else None
        return _waited(self, [((n_rows,), np.float64), hop_sums, ((n_rows,), np.uint32)],
                       lambda g, h, b: call(rows_dev, row_stride, len_dev, n_rows, sample_rate, coef, g, h, hs if hops else 0, b))

    def true_peak_async(self, rows_dev, row_stride, len_dev, n_rows, true_peak_dev=None, nonfinite_dev=None):
        """grail_true_peak_async: per row the true peak (4x oversampled, BS.1770-4 Annex 2) and the count of non-finite
        samples, into DEVICE arrays [n_rows] (either may be None), queued on the context's stream."""
        _check(load().grail_true_peak_async(self.handle, rows_dev, row_stride, len_dev, n_rows, true_peak_dev,
                                            nonfinite_dev))

    def true_peak(self, rows_dev, row_stride, len_dev, n_rows):
        """true_peak_async, waited for and copied back: (true_peak float64, nonfinite uint32), one per row."""
        return _waited(self, _per(n_rows, np.float64, np.uint32),
                       lambda *d: self.true_peak_async(rows_dev, row_stride, len_dev, n_rows, *d))

    def limit_async(self, rows_dev, row_stride, len_dev, n_rows, ceiling, lookahead_log2, out_dev, out_stride=None, group=1,
                    min_gain_dev=None, n_limited_dev=None, nonfinite_dev=None):
        """grail_limit_async: the look-ahead limiter over groups of `group` consecutive rows, into out_dev (must not overlap
        rows_dev); ceiling is linear (limit_ceiling gives it from dBTP), the look-ahead 2^lookahead_log2 samples.  Results
        are DEVICE arrays [n_rows // group] (any may be None), queued on the context's stream."""
        _check(load().grail_limit_async(self.handle, rows_dev, row_stride, len_dev, n_rows, group, float(np.float32(ceiling)),
                                        lookahead_log2, out_dev, row_stride if out_stride is None else out_stride,
                                        min_gain_dev, n_limited_dev, nonfinite_dev))

    def limit(self, rows_dev, row_stride, len_dev, n_rows, ceiling, lookahead_log2, out_dev, out_stride=None, group=1):
        """limit_async, waited for, the results copied back: (min_gain float32, n_limited uint32, nonfinite uint32), one per
        group; a refused group reads (NaN, LIMIT_REFUSED, 0)."""
        return _waited(self, _per(n_rows // group if group else 0, np.float32, np.uint32, np.uint32),
                       lambda *d: self.limit_async(rows_dev, row_stride, len_dev, n_rows, ceiling, lookahead_log2, out_dev,
                                                   out_stride, group, *d))

    def resample_async(self, rows_dev, row_stride, len_dev, n_rows, rate_in, rate_out, out_dev, out_stride, out_len_dev=None,
                       nonfinite_dev=None):
        """grail_resample_async: the rows at rate_in resampled to rate_out into out_dev (must not overlap rows_dev), output m
        at input time m * down / up.  Results are DEVICE arrays [n_rows] (either may be None), queued on the context's
        stream."""
        _check(load().grail_resample_async(self.handle, rows_dev, row_stride, len_dev, n_rows, rate_in, rate_out, out_dev,
                                           out_stride, out_len_dev, nonfinite_dev))

    def resample(self, rows_dev, row_stride, len_dev, n_rows, rate_in, rate_out, out_dev, out_stride):
        """resample_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32),
                       lambda *d: self.resample_async(rows_dev, row_stride, len_dev, n_rows, rate_in, rate_out, out_dev,
                                                      out_stride, *d))

    def fir_create(self, filters):
        """grail_fir_create: a set of filters on this context's device.  filters: a list of (taps float32[K], origin), one per
        filter.  Returns the set's handle, for fir / fir_async / fir_free; sets still alive go with the context."""
        taps = [np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t, _ in filters]
        flat = np.concatenate(taps) if taps else np.zeros(0, np.float32)
        n_taps = np.array([len(t) for t in taps], dtype=np.uint32)
        origin = np.array([o for _, o in filters], dtype=np.uint32)
        out = C.c_void_p(None)
        _check(load().grail_fir_create(self.handle, flat.ctypes.data, n_taps.ctypes.data, origin.ctypes.data, len(filters),
                                       C.addressof(out)))
        return out

    def fir_free(self, fir_set):
        """grail_fir_free: waits for the context's stream, then releases the set."""
        _check(load().grail_fir_free(self.handle, fir_set))

    def fir_async(self, fir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, out_dev, out_stride, out_len_dev=None,
                  nonfinite_dev=None):
        """grail_fir_async: the rows filtered into out_dev (must not overlap rows_dev), row u with filter filter_dev[u] of the
        set (a DEVICE array of uint32; None: filter 0 for every row).  Results are DEVICE arrays [n_rows] (either may be
        None), queued on the context's stream."""
        _check(load().grail_fir_async(self.handle, fir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, out_dev, out_stride,
                                      out_len_dev, nonfinite_dev))

    def fir(self, fir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, out_dev, out_stride):
        """fir_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row whose
        filter index is outside the set: (LIMIT_REFUSED, 0)."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32),
                       lambda *d: self.fir_async(fir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, out_dev, out_stride,
                                                 *d))

    def fir_stream_open(self, fir_set, n_rows, filters=None):
        """grail_filter_stream_open: a stream of n_rows rows filtered call by call, row u bound to filter filters[u] of the set
        (a host sequence; None: filter 0 for every row).  Returns the stream's handle, for fir_stream_next / _finish /
        _close; streams still open go with the context, and their set cannot be freed before them."""
        which = _arr(filters, np.uint32)
        out = C.c_void_p(None)
        _check(load().grail_filter_stream_open(self.handle, fir_set, n_rows, _ptr(which), C.addressof(out)))
        return out

    def fir_stream_next_async(self, fs, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None, nonfinite_dev=None):
        """grail_filter_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples; the outputs that
        became known go to out_dev + u * out_stride.  Results are DEVICE arrays [n_rows] (either may be None), queued on the
        context's stream; in_dev may be reused by what is queued behind the call."""
        _check(load().grail_filter_stream_next_async(self.handle, fs, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev,
                                                     nonfinite_dev))

    def fir_stream_next(self, fs, n_rows, in_dev, in_stride, in_len_dev, out_dev, out_stride):
        """fir_stream_next_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row
        that had ended and was fed: (LIMIT_REFUSED, 0)."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32),
                       lambda *d: self.fir_stream_next_async(fs, in_dev, in_stride, in_len_dev, out_dev, out_stride, *d))

    def _stream_finish(self, finish_async, st, n_rows, out_dev, out_stride, which, out_len_dev):
        """A `*_stream_finish_async` of the library in its two modes: out_len_dev given, queued; None, waited for, and the
        tails' lengths returned."""
        marks = _marks(which, n_rows)

        def finish(out_len):
            _check(finish_async(self.handle, st, _ptr(marks), out_dev, out_stride, out_len))
        return finish(out_len_dev) if out_len_dev is not None else _waited(self, _per(n_rows, np.uint32), finish)[0]

    def fir_stream_finish(self, fs, n_rows, out_dev, out_stride, which=None, out_len_dev=None):
        """grail_filter_stream_finish_async: the rows marked in which (a host sequence, non-zero = marked; None: every row)
        that have not ended write their tails and end.  out_len_dev None: waited for, and the tails' lengths (uint32, one
        per row; 0 for rows not marked or ended before) returned."""
        return self._stream_finish(load().grail_filter_stream_finish_async, fs, n_rows, out_dev, out_stride, which, out_len_dev)

    def fir_stream_close(self, fs):
        """grail_filter_stream_close: waits for the context's stream, then releases the stream."""
        _check(load().grail_filter_stream_close(self.handle, fs))

    def iir_create(self, filters):
        """grail_iir_create: a set of recursive filters on this context's device.  filters: a list of float64 arrays [S][5]
        (or flat [5 S]), the sections b0 b1 b2 a1 a2 of one filter each.  Returns the set's handle, for iir / iir_async /
        iir_free / iir_stream_open; sets still alive go with the context."""
        secs = [np.ascontiguousarray(f, dtype=np.float64).reshape(-1) for f in filters]
        flat = np.concatenate(secs) if secs else np.zeros(0, np.float64)
        n_sections = np.array([len(f) // 5 for f in secs], dtype=np.uint32)
        assert all(len(f) % 5 == 0 for f in secs)
        out = C.c_void_p(None)
        _check(load().grail_iir_create(self.handle, flat.ctypes.data, n_sections.ctypes.data, len(filters), C.addressof(out)))
        return out

    def iir_free(self, iir_set):
        """grail_iir_free: waits for the context's stream, then releases the set (refused while it has open streams)."""
        _check(load().grail_iir_free(self.handle, iir_set))

    def iir_async(self, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev, out_stride, out_len_dev=None,
                  nonfinite_dev=None):
        """grail_iir_async: the rows filtered into out_dev (must not overlap rows_dev), row u with filter filter_dev[u] of the
        set (a DEVICE array of uint32; None: filter 0 for every row), ringing out over `tail` outputs past its last sample.
        Results are DEVICE arrays [n_rows] (either may be None), queued on the context's stream."""
        _check(load().grail_iir_async(self.handle, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev,
                                      out_stride, out_len_dev, nonfinite_dev))

    def iir(self, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev, out_stride):
        """iir_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row whose
        filter index is outside the set: (LIMIT_REFUSED, 0)."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32),
                       lambda *d: self.iir_async(iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev,
                                                 out_stride, *d))

    def iir_blocked_async(self, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev, out_stride,
                          out_len_dev=None, nonfinite_dev=None):
        """grail_biquad_blocked_async: iir_async's arguments and results, parallel in time: a row's steps in blocks of IIR_BLOCK,
        a lane each.  The call for a few long rows; bit for bit iir_async's up to a row's IIR_BLOCK-th output, its own
        contract from there on."""
        _check(load().grail_biquad_blocked_async(self.handle, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail,
                                              out_dev, out_stride, out_len_dev, nonfinite_dev))

    def iir_blocked(self, iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail, out_dev, out_stride):
        """iir_blocked_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row
        whose filter index is outside the set: (LIMIT_REFUSED, 0)."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32),
                       lambda *d: self.iir_blocked_async(iir_set, rows_dev, row_stride, len_dev, n_rows, filter_dev, tail,
                                                         out_dev, out_stride, *d))

    def iir_stream_open(self, iir_set, n_rows, filters=None, tail=0):
        """grail_iir_stream_open: a stream of n_rows rows filtered recursively call by call, row u bound to filter filters[u]
        of the set (a host sequence; None: filter 0 for every row), every row ringing out over `tail` outputs at its finish.
        Returns the stream's handle, for iir_stream_next / _finish / _close."""
        which = _arr(filters, np.uint32)
        out = C.c_void_p(None)
        _check(load().grail_iir_stream_open(self.handle, iir_set, n_rows, _ptr(which), tail, C.addressof(out)))
        return out

    def iir_stream_next_async(self, st, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None, nonfinite_dev=None):
        """grail_iir_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples and writes as many
        outputs to out_dev + u * out_stride.  Results are DEVICE arrays [n_rows] (either may be None)."""
        _check(load().grail_iir_stream_next_async(self.handle, st, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev,
                                                  nonfinite_dev))

    def iir_stream_next(self, st, n_rows, in_dev, in_stride, in_len_dev, out_dev, out_stride):
        """iir_stream_next_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a row
        that had ended and was fed: (LIMIT_REFUSED, 0)."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32),
                       lambda *d: self.iir_stream_next_async(st, in_dev, in_stride, in_len_dev, out_dev, out_stride, *d))

    def iir_stream_finish(self, st, n_rows, out_dev, out_stride, which=None, out_len_dev=None):
        """grail_iir_stream_finish_async: the rows marked in which (a host sequence, non-zero = marked; None: every row) that
        have not ended write their tails and end.  out_len_dev None: waited for, and the tails' lengths (uint32, one per row;
        0 for rows not marked, ended before or fed nothing) returned."""
        return self._stream_finish(load().grail_iir_stream_finish_async, st, n_rows, out_dev, out_stride, which, out_len_dev)

    def iir_stream_close(self, st):
        """grail_iir_stream_close: waits for the context's stream, then releases the stream."""
        _check(load().grail_iir_stream_close(self.handle, st))

    def dyn_create(self, curves):
        """grail_dyn_create: a set of gain curves on this context's device.  curves: a list of (gain float64[DYN_POINTS], (alpha_attack,
        alpha_release), detector), as dyn_design and dyn_ballistics return them or the caller's own.  Returns the set's handle, for
        dyn / dyn_async / dyn_free / dyn_stream_open; sets still alive go with the context."""
        gain = np.ascontiguousarray([np.asarray(c[0], dtype=np.float64) for c in curves], dtype=np.float64).reshape(-1)
        assert len(gain) == DYN_POINTS * len(curves)
        alpha = np.ascontiguousarray([c[1] for c in curves], dtype=np.float64).reshape(-1)
        detector = np.array([c[2] for c in curves], dtype=np.uint32)
        out = C.c_void_p(None)
        _check(load().grail_dyn_create(self.handle, gain.ctypes.data, alpha.ctypes.data, detector.ctypes.data, len(curves),
                                       C.addressof(out)))
        return out

    def dyn_free(self, dyn_set):
        """grail_dyn_free: waits for the context's stream, then releases the set (refused while it has open streams)."""
        _check(load().grail_dyn_free(self.handle, dyn_set))

    def dyn_async(self, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride, out_len_dev=None,
                  nonfinite_dev=None, min_gain_dev=None, key_dev=None, key_stride=0, key_len_dev=None, n_keys=0, key_row_dev=None):
        """grail_dyn_async: the rows times the gain their curve (curve_dev: a DEVICE array of uint32; None: curve 0 for every row)
        gives at their envelope, into out_dev (must overlap neither rows_dev nor the keys).  key_dev None: every row follows
        itself; else row u follows key key_row_dev[u] (None: key u) of the n_keys rows at key_dev.  Results are DEVICE arrays
        [n_rows] (each may be None; min_gain is float64), queued on the context's stream."""
        _check(load().grail_dyn_async(self.handle, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, key_dev, key_stride,
                                      key_len_dev, n_keys, key_row_dev, out_dev, out_stride, out_len_dev, nonfinite_dev, min_gain_dev))

    def dyn(self, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride, key_dev=None, key_stride=0,
            key_len_dev=None, n_keys=0, key_row_dev=None):
        """dyn_async, waited for, the results copied back: (out_len uint32, nonfinite uint32, min_gain float64), one per row; a
        row whose curve or key index is outside: (LIMIT_REFUSED, 0, NaN)."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32, np.float64),
                       lambda *d: self.dyn_async(dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride,
                                                 *d, key_dev=key_dev, key_stride=key_stride, key_len_dev=key_len_dev,
                                                 n_keys=n_keys, key_row_dev=key_row_dev))

    def track_dyn_async(self, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride, out_len_dev=None,
                        nonfinite_dev=None, min_gain_dev=None, key_dev=None, key_stride=0, key_len_dev=None, n_keys=0, key_row_dev=None):
        """grail_track_dyn_async: dyn_async's arguments, results and bits with a workgroup a row, for the few long tracks of a
        mix (the header's WHICH CALL FOR WHAT says below how many rows)."""
        _check(load().grail_track_dyn_async(self.handle, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, key_dev, key_stride,
                                            key_len_dev, n_keys, key_row_dev, out_dev, out_stride, out_len_dev, nonfinite_dev,
                                            min_gain_dev))

    def track_dyn(self, dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev, out_stride, key_dev=None, key_stride=0,
                  key_len_dev=None, n_keys=0, key_row_dev=None):
        """track_dyn_async, waited for, the results copied back as dyn does: (out_len uint32, nonfinite uint32, min_gain
        float64), one per row."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32, np.float64),
                       lambda *d: self.track_dyn_async(dyn_set, rows_dev, row_stride, len_dev, n_rows, curve_dev, out_dev,
                                                       out_stride, *d, key_dev=key_dev, key_stride=key_stride,
                                                       key_len_dev=key_len_dev, n_keys=n_keys, key_row_dev=key_row_dev))

    def dyn_stream_open(self, dyn_set, n_rows, curves=None, n_keys=0, key_rows=None):
        """grail_dyn_stream_open: a stream of n_rows rows compressed call by call, row u bound to curve curves[u] of the set (a
        host sequence; None: curve 0 for every row).  n_keys = 0: every row follows itself; else row u follows key key_rows[u]
        (a host sequence; None: key u) of the n_keys key rows each call brings.  Returns the stream's handle, for
        dyn_stream_next / _close."""
        which, keys = _arr(curves, np.uint32), _arr(key_rows, np.uint32)
        assert (which is None or len(which) == n_rows) and (keys is None or len(keys) == n_rows)
        out = C.c_void_p(None)
        _check(load().grail_dyn_stream_open(self.handle, dyn_set, n_rows, _ptr(which), n_keys, _ptr(keys), C.addressof(out)))
        return out

    def dyn_stream_next_async(self, st, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None, nonfinite_dev=None,
                              min_gain_dev=None, key_dev=None, key_stride=0):
        """grail_dyn_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples (and, keyed, reads as many
        of its key at key_dev) and writes as many outputs to out_dev + u * out_stride.  Results are DEVICE arrays [n_rows] (each
        may be None; min_gain is float64)."""
        _check(load().grail_dyn_stream_next_async(self.handle, st, in_dev, in_stride, in_len_dev, key_dev, key_stride, out_dev,
                                                  out_stride, out_len_dev, nonfinite_dev, min_gain_dev))

    def dyn_stream_next(self, st, n_rows, in_dev, in_stride, in_len_dev, out_dev, out_stride, key_dev=None, key_stride=0):
        """dyn_stream_next_async, waited for, the results copied back: (out_len uint32, nonfinite uint32, min_gain float64), one
        per row."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32, np.float64),
                       lambda *d: self.dyn_stream_next_async(st, in_dev, in_stride, in_len_dev, out_dev, out_stride, *d,
                                                             key_dev=key_dev, key_stride=key_stride))

    def dyn_stream_close(self, st):
        """grail_dyn_stream_close: waits for the context's stream, then releases the stream."""
        _check(load().grail_dyn_stream_close(self.handle, st))

    def resample_stream_open(self, rate_in, rate_out, n_rows):
        """grail_resample_stream_open: a stream of n_rows rows resampled call by call from rate_in to rate_out.  Returns the
        stream's handle, for resample_stream_next / _finish / _close; streams still open go with the context."""
        out = C.c_void_p(None)
        _check(load().grail_resample_stream_open(self.handle, rate_in, rate_out, n_rows, C.addressof(out)))
        return out

    def resample_stream_next_async(self, rs, in_dev, in_stride, in_len_dev, out_dev, out_stride, out_len_dev=None,
                                   nonfinite_dev=None):
        """grail_resample_stream_next_async: every row is fed its next min(in_len_dev[u], in_stride) samples; the outputs that
        became known go to out_dev + u * out_stride (out_stride >= resample_len(in_stride)).  Results are DEVICE arrays
        [n_rows] (either may be None), queued on the context's stream; in_dev may be reused by what is queued behind the call."""
        _check(load().grail_resample_stream_next_async(self.handle, rs, in_dev, in_stride, in_len_dev, out_dev, out_stride,
                                                       out_len_dev, nonfinite_dev))

    def resample_stream_next(self, rs, n_rows, in_dev, in_stride, in_len_dev, out_dev, out_stride):
        """resample_stream_next_async, waited for, the results copied back: (out_len uint32, nonfinite uint32), one per row; a
        row that had ended and was fed: (LIMIT_REFUSED, 0)."""
        return _waited(self, _per(n_rows, np.uint32, np.uint32),
                       lambda *d: self.resample_stream_next_async(rs, in_dev, in_stride, in_len_dev, out_dev, out_stride, *d))

    def resample_stream_finish(self, rs, n_rows, out_dev, out_stride, which=None, out_len_dev=None):
        """grail_resample_stream_finish_async: the rows marked in which (a host sequence, non-zero = marked; None: every row)
        that have not ended write their tails and end.  out_len_dev None: waited for, and the tails' lengths (uint32, one
        per row; 0 for rows not marked or ended before) returned."""
        return self._stream_finish(load().grail_resample_stream_finish_async, rs, n_rows, out_dev, out_stride, which, out_len_dev)

    def resample_stream_close(self, rs):
        """grail_resample_stream_close: waits for the context's stream, then releases the stream."""
        _check(load().grail_resample_stream_close(self.handle, rs))

    def limit_stream_open(self, n_rows, ceiling, lookahead_log2, group=1):
        """grail_limit_stream_open: a stream of n_rows rows in groups of `group`, limited call by call under `ceiling` (linear)
        with a look-ahead of 2^lookahead_log2 samples.  Returns a LimitStream; streams still open go with the context."""
        out = C.c_void_p(None)
        _check(load().grail_limit_stream_open(self.handle, n_rows, group, float(np.float32(ceiling)), lookahead_log2, C.addressof(out)))
        return LimitStream(self, out, n_rows, group, lookahead_log2)

    def meter_stream_open(self, n_rows, sample_rate, max_hops, coef=None):
        """grail_meter_stream_open: a stream of n_rows rows metered call by call at sample_rate (coef: float64 [10], None:
        kweighting(sample_rate)), each row's ledger holding max_hops hops.  Returns a MeterStream; streams still open go
        with the context."""
        out = C.c_void_p()
        c = _coef10(coef)
        _check(load().grail_meter_stream_open(self.handle, n_rows, int(sample_rate), _ptr(c), int(max_hops), C.addressof(out)))
        return MeterStream(self, out, n_rows, int(sample_rate), int(max_hops))

    def digest(self, in_dev, in_stride, len_dev, n_utt):
        """(bit-pattern sums mod 2^64, max finite |x|, non-finite counts) per row, computed on the device (every length
        at most the stride).  A sum is blind to samples permuted within a row: use compare beside it."""
        sums = np.zeros(max(n_utt, 1), dtype=np.uint64)
        maxabs = np.zeros(max(n_utt, 1), dtype=np.float32)
        bad = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_batch_digest(self.handle, in_dev, in_stride, len_dev, n_utt,
                                         sums.ctypes.data, maxabs.ctypes.data, bad.ctypes.data))
        return sums[:n_utt], maxabs[:n_utt], bad[:n_utt]

    def compare(self, a_dev, b_dev, stride, len_a_dev, len_b_dev, n_utt):
        """(max |a-b|, sum (a-b)^2, structural mismatches) per row of two device renderings, over the first len_a samples
        (every length at most the stride).  A sample whose |a-b| is not finite enters neither number and is a mismatch
        unless both sides carry the same bits or both are NaN; +1 where the lengths differ; -0.0 equals +0.0."""
        md = np.zeros(max(n_utt, 1), dtype=np.float32)
        sq = np.zeros(max(n_utt, 1), dtype=np.float64)
        bad = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_batch_compare(self.handle, a_dev, b_dev, stride, len_a_dev, len_b_dev, n_utt,
                                          md.ctypes.data, sq.ctypes.data, bad.ctypes.data))
        return md[:n_utt], sq[:n_utt], bad[:n_utt]

    def h2d(self, dst_dev, src, nbytes):
        _check(load().grail_memcpy_h2d(self.handle, dst_dev, src.ctypes.data, nbytes))

    def sync(self):
        _check(load().grail_sync(self.handle))

    def last_kernel_ms(self):
        ms = C.c_float()
        _check(load().grail_last_kernel_ms(self.handle, C.byref(ms)))
        return ms.value

    def last_kernel_name(self):
        return load().grail_last_kernel_name(self.handle).decode()

    def device_alloc(self, nbytes):
        p = C.c_void_p()
        _check(load().grail_device_alloc(self.handle, nbytes, C.byref(p)))
        return p

    def device_free(self, p):
        _check(load().grail_device_free(self.handle, p))

    def host_alloc(self, shape, dtype):
        """A numpy array in pinned host memory (grail_host_alloc); free it with host_free(array)."""
        return _pinned_array(self, load().grail_host_alloc, shape, dtype)

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        _check(load().grail_host_free(self.handle, p))

    def synthesize_into(self, out, out_len, segs, seg_offsets, voice_ids=None, jitter_seeds=None):
        """One-call form into a caller-owned host array out[n_utt, out_stride] (f32 or i16)."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = self._prep(None, segs, seg_offsets, voice_ids,
                                                                 jitter_seeds)
        assert out.shape[0] >= n_utt and out.flags.c_contiguous
        fn = load().grail_synthesize_batch if out.dtype == np.float32 else load().grail_synthesize_batch_pcm16
        _check(fn(self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids), _ptr(jitter_seeds),
                  n_utt, out.ctypes.data, out.shape[1], out_len.ctypes.data, OUT_HOST))

    def d2h(self, dst, src_dev, nbytes, offset=0):
        src = C.c_void_p(src_dev.value + offset)
        _check(load().grail_memcpy_d2h(self.handle, dst.ctypes.data, src, nbytes))

    def memset(self, dst_dev, value, nbytes):
        _check(load().grail_memset_d(self.handle, dst_dev, value, nbytes))

    # RCCL
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        _check(load().grail_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        _check(load().grail_comm_init(self.handle, buf, rank, world))

    def broadcast_voices(self, n_voices, root=0):
        _check(load().grail_broadcast_voices(self.handle, n_voices, root))

    def comm_info(self):
        """(ncclCommCount, ncclCommUserRank) of this context's communicator; (0, 0) without one."""
        n, r = C.c_uint32(), C.c_uint32()
        _check(load().grail_comm_info(self.handle, C.byref(n), C.byref(r)))
        return n.value, r.value


def _pinned_array(owner, alloc, shape, dtype):
    """host_alloc of a Context or a Node: a numpy array over pinned memory from `alloc`, remembered by its address for
    host_free"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    p = C.c_void_p()
    _check(alloc(owner.handle, n, C.byref(p)))
    buf = (C.c_char * max(n, 1)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    owner._pinned = getattr(owner, "_pinned", {})
    owner._pinned[arr.ctypes.data] = p
    return arr


class _BorrowedContext(Context):
    """A node's context (grail_node_context): owned by the node, never destroyed from here."""

    def __init__(self, handle, device):       # noqa: super().__init__ would create a context
        self.handle, self.device = handle, device

    def close(self):
        self.handle = None


class Node:
    """grail_node: one process, several GPUs — a context and a host thread per device; one call renders a batch over all
    of them (contiguous shards, no data-path collective; the voice table travels by one ncclBroadcast)."""

    def __init__(self, devices, voices_without_rccl=False):
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        _check(load().grail_node_create(arr, len(self.devices), C.byref(h)))
        self.handle = h
        if voices_without_rccl:
            self.set_option("node_voices_without_rccl", 1)

    def close(self):
        if self.handle:
            load().grail_node_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def size(self):
        return int(load().grail_node_size(self.handle))

    def context(self, index):
        h = C.c_void_p()
        _check(load().grail_node_context(self.handle, index, C.byref(h)))
        return _BorrowedContext(h, self.devices[index])

    def set_voices(self, voices):
        arr = (Voice * len(voices))(*[v.copy() for v in voices])
        _check(load().grail_node_set_voices(self.handle, C.cast(arr, C.c_void_p), len(voices)))

    def set_option(self, name, value):
        _check(load().grail_node_set_option(self.handle, name.encode(), value))

    def get_option(self, name):
        v = C.c_int64()
        _check(load().grail_node_get_option(self.handle, name.encode(), C.byref(v)))
        return v.value

    def lengths(self, segs, seg_offsets, voice_ids=None, max_len=0xFFFFFFFF):
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, _ = Context._prep(None, segs, seg_offsets, voice_ids, None)
        out = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_node_lengths(self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids), n_utt,
                                         max_len, out.ctypes.data))
        return out[:n_utt]

    def synthesize(self, segs, seg_offsets, voice_ids=None, jitter_seeds=None, out_stride=None, out=None,
                   allow_truncation=False, pcm16=False):
        """grail_node_synthesize_batch(_pcm16) over host buffers.  Returns (out[n_utt, out_stride], out_len)."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = Context._prep(None, segs, seg_offsets, voice_ids, jitter_seeds)
        if out is not None:
            out_stride = out.shape[1]
            assert out.shape[0] >= n_utt and out.flags.c_contiguous
            pcm16 = out.dtype == np.int16
        elif out_stride is None:
            lens = self.lengths(segs, seg_offsets, voice_ids)
            out_stride = int((max(int(lens.max()) if n_utt else 0, 1) + 63) // 64 * 64)
        if out is None:
            out = np.zeros((max(n_utt, 1), out_stride), dtype=np.int16 if pcm16 else np.float32)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        fn = load().grail_node_synthesize_batch_pcm16 if pcm16 else load().grail_node_synthesize_batch
        st = fn(self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids), _ptr(jitter_seeds), n_utt,
                out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST)
        if not (allow_truncation and st == ERR_BUFFER_TOO_SMALL):
            _check(st)
        return out[:n_utt], out_len[:n_utt]

    def synthesize_device(self, segs, seg_offsets, voice_ids, jitter_seeds, out_dev, out_stride):
        """grail_node_synthesize_batch_device: slot i's shard into out_dev[i] (device memory of its GPU).  Returns out_len."""
        segs = np.ascontiguousarray(segs, dtype=PHONEME_DTYPE)
        seg_offsets, n_utt, voice_ids, jitter_seeds = Context._prep(None, segs, seg_offsets, voice_ids, jitter_seeds)
        ptrs = (C.c_void_p * self.size())(*[p if p is None or isinstance(p, C.c_void_p) else C.c_void_p(p) for p in out_dev])
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_node_synthesize_batch_device(self.handle, segs.ctypes.data, seg_offsets.ctypes.data, _ptr(voice_ids),
                                                         _ptr(jitter_seeds), n_utt, ptrs, out_stride, out_len.ctypes.data))
        return out_len[:n_utt]

    def synthesize_elems(self, seq_elems, seg_offsets, voice_ids=None, jitter_seeds=None, out_stride=4096):
        arr = (SequenceElem * max(len(seq_elems), 1))(*seq_elems)
        seg_offsets, n_utt, voice_ids, jitter_seeds = Context._prep(None, None, seg_offsets, voice_ids, jitter_seeds)
        out = np.zeros((max(n_utt, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n_utt, 1), dtype=np.uint32)
        _check(load().grail_node_synthesize_batch_elems(
            self.handle, C.cast(arr, C.c_void_p), seg_offsets.ctypes.data, _ptr(voice_ids), _ptr(jitter_seeds), n_utt,
            out.ctypes.data, out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n_utt], out_len[:n_utt]

    def say(self, texts, voice_ids=None, jitter_seeds=None, out_stride=4096):
        n = len(texts)
        arr = (C.c_char_p * max(n, 1))(*[t.encode("utf-8") for t in texts])
        voice_ids, jitter_seeds = _arr(voice_ids, np.uint32), _arr(jitter_seeds, np.uint32)
        out = np.zeros((max(n, 1), out_stride), dtype=np.float32)
        out_len = np.zeros(max(n, 1), dtype=np.uint32)
        _check(load().grail_node_say_batch(self.handle, arr, n, _ptr(voice_ids), _ptr(jitter_seeds), out.ctypes.data,
                                           out_stride, out_len.ctypes.data, OUT_HOST))
        return out[:n], out_len[:n]

    def last_shard_ms(self):
        ms = (C.c_float * self.size())()
        _check(load().grail_node_last_shard_ms(self.handle, ms, self.size()))
        return [float(x) for x in ms]

    def host_alloc(self, shape, dtype):
        """A numpy array in pinned host memory every device of the node can copy into; free it with host_free(array)."""
        return _pinned_array(self, load().grail_node_host_alloc, shape, dtype)

    def host_free(self, arr):
        p = self._pinned.pop(arr.ctypes.data)
        _check(load().grail_node_host_free(self.handle, p))
