"""Where a rendering may store (include/grail_hip.h: grail_batch_synthesize_async, grail_stream_next_async, the one-call
GRAIL_OUT_HOST forms): a small ragged corpus, the oracle's rows of it, and device buffers with canary words around every
row, in front of the first and behind the last.  A plain helper module for tests/test_store_footprint_gpu.py; it holds no
test and no fixture.  Nothing here needs a GPU until a function is handed a context."""
import ctypes as C

import numpy as np

import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W

GUARD = 8                      # rows in front of and behind the batch's own; a multiple of 8: the first row keeps the
                               # allocation's alignment (16 bytes and more) for f32 and i16 rows of every stride
CANARY = 0x7FC0DEAD            # f32 rows: a quiet NaN no arithmetic of the kernels produces
CANARY16 = 0x5A5A              # i16 rows
LEN_CANARY = 0xDEADBEEF        # around out_len
LEN_GUARD = 64                 # words in front of and behind out_len
RATE = 48000.0
N_UTT = 200
CAPACITIES = (1024, 1021, 61)  # strides that cut rows: at a whole tile, inside a tile (odd), below one 64-sample tile
VARIANTS = ("lean4", "lean4_anybl", "live8", "odd")
_cache = {}


def ovoices(voices):
    return [O.Voice.from_buffer_copy(bytes(v)) for v in voices]


def pcm16_of(x):
    """examples/cli.rs:49, `(x * i16::MAX as f32) as i16` (a saturating cast; NaN gives 0)."""
    v = x.astype(np.float32) * np.float32(32767.0)
    return np.where(np.isnan(v), 0, np.clip(np.trunc(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9)), -32768, 32767)).astype(np.int16)


def _segments(rng, n_utt, any_blend, odd):
    """n_utt utterances of 1 - 5 segments; a segment lasts 0.5 - 30 ms or 2^-5 ... 2^-8 s, blends over 2^-5 ... 2^-8 s (or,
    any_blend, over 3 - 30 ms), at 90 - 220 Hz.  Row 0 is the longest the recipe gives (five segments of 2^-5 s); rows 6,
    64, 127 and 198 are one segment of 24 - 52 samples: shorter than a tile, whole under the smallest capacity.
    odd: the rows the lean kernel families do not take — one without segments, rows of 1, 2 and 3 samples (one segment of
    (k + 0.5) / 48000 s), zero-length segments inside rows, Stop and Glide among the phonemes."""
    phonemes = [G.PH_A, G.PH_E, G.PH_SILENCE] + ([G.PH_STOP, G.PH_GLIDE] if odd else [])
    utts = []
    for u in range(n_utt):
        k = int(rng.integers(1, 6))
        utt = []
        for i in range(k):
            length = float(rng.uniform(0.0005, 0.030)) if rng.random() < 0.7 else float(2.0 ** -rng.integers(5, 9))
            blend = float(rng.uniform(0.003, 0.030)) if any_blend else float(2.0 ** -rng.integers(5, 9))
            ph = G.PH_SILENCE if i == 0 and not odd else int(rng.choice(phonemes))
            utt.append((ph, length, blend, float(rng.uniform(90.0, 220.0) / RATE)))
        utts.append(utt)
    utts[0] = [(utts[0][0][0] if i == 0 else (G.PH_A, G.PH_E)[i % 2], 2.0 ** -5, utts[0][0][2], 120.0 / RATE) for i in range(5)]
    for k, u in enumerate((6, 64, 127, 198)):      # rows shorter than one tile (a capacity of 61 leaves them whole)
        utts[u] = [(G.PH_E, (24.5 + 9 * k) / RATE, utts[u][0][2], utts[u][0][3])]
    if odd:
        f = 110.0 / RATE
        utts[1] = []
        for k in (1, 2, 3):
            utts[1 + k] = [(G.PH_A, (k + 0.5) / RATE, 2.0 ** -6, f)]
        for u in (5, 70, 131, 199):          # a zero-length segment first, inside and last
            at = (0, len(utts[u]) // 2, len(utts[u]) - 1, 0)[u % 4]
            utts[u][at] = (utts[u][at][0], 0.0, utts[u][at][2], utts[u][at][3])
    return utts


def corpus(variant, repeat=1):
    """(voices, segs, offs, vids, seeds, ref, ref_len, S) of a variant, computed once and read-only afterwards: ref[u] is
    the oracle's row u at stride S (the longest row rounded up to 64 samples, and 64 more where that leaves it no tail),
    ref_len[u] its uncut length.  A launch that cuts rows at a capacity renders a prefix of the same rows.
    repeat > 1: the variant's rows `repeat` times over with fresh seeds (launches that need more rows than 200)."""
    key = (variant, repeat)
    if key not in _cache:
        assert variant in VARIANTS, variant
        rng = np.random.default_rng(5 + VARIANTS.index(variant))
        voices = W.preset_voices(8) if variant == "live8" else W.single_voice()
        utts = _segments(rng, N_UTT, variant == "lean4_anybl", variant == "odd") * repeat
        n_utt = len(utts)
        segs = G.segments([s for u in utts for s in u])
        offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32)
        vids = (np.arange(n_utt) % len(voices)).astype(np.uint32)
        seeds = rng.integers(0, 2 ** 32, n_utt, dtype=np.uint64).astype(np.uint32)
        lens = O.count_batch(ovoices(voices), segs, offs, vids, seeds)
        S = (int(lens.max()) + 63) // 64 * 64
        S += 64 if S == int(lens.max()) else 0
        ref, ref_len = O.synthesize_batch(ovoices(voices), segs, offs, vids, seeds, S)
        assert np.array_equal(ref_len, lens)
        for a in (segs, offs, vids, seeds, ref, ref_len):
            a.setflags(write=False)
        _cache[key] = (voices, segs, offs, vids, seeds, ref, ref_len, S)
    return _cache[key]


def first_rows(c, n):
    """The first n rows of a corpus (same rows, same oracle, same S)."""
    voices, segs, offs, vids, seeds, ref, ref_len, S = c
    if n is None or n >= len(ref_len):
        return c
    return voices, segs[:offs[n]], offs[:n + 1], vids[:n], seeds[:n], ref[:n], ref_len[:n], S


def as_sequence_elems(voices, segs, offs, vids):
    """The PhonemeElems of a batch as the SequenceElems the Selector would hand on (src/lib.rs:990-1005)."""
    arr = (G.SequenceElem * max(len(segs), 1))()
    for u in range(len(offs) - 1):
        v = voices[int(vids[u])]
        for i in range(int(offs[u]), int(offs[u + 1])):
            ph = int(segs["phoneme"][i])
            arr[i].has_elem = 1 if ph >= G.PH_A else 0
            if ph >= G.PH_A:
                arr[i].elem = v.phonemes[ph - G.PH_A]
            arr[i].elem.frequency = min(float(segs["frequency"][i]), 0.5)
            arr[i].length = float(segs["length"][i])
            arr[i].blend_length = float(segs["blend_length"][i])
    return arr


def sequence_oracle(c):
    """(ref, ref_len) of a corpus rendered by the oracle from caller-built SequenceElems, row by row, at the corpus' S."""
    key = ("elems", id(c[5]))
    if key not in _cache:
        voices, segs, offs, vids, seeds, _, _, S = c
        arr = as_sequence_elems(voices, segs, offs, vids)
        ov = ovoices(voices)
        n_utt = len(offs) - 1
        ref, ref_len = np.zeros((n_utt, S), dtype=np.float32), np.zeros(n_utt, dtype=np.uint32)
        for u in range(n_utt):
            elems = [O.SequenceElem.from_buffer_copy(bytes(arr[i])) for i in range(int(offs[u]), int(offs[u + 1]))]
            row = O.synthesize_sequence(ov[int(vids[u])], elems, int(seeds[u]))
            ref[u, :len(row)], ref_len[u] = row, len(row)
        ref.setflags(write=False)
        ref_len.setflags(write=False)
        _cache[key] = (arr, ref, ref_len)
    return _cache[key]


class Guarded:
    """Device memory for one launch: GUARD rows, n_utt rows, GUARD rows of `stride` f32 or i16 samples, every word a canary,
    the first row base_offset bytes into the allocation (0, or one sample: 4 bytes for f32, 2 for i16); out_len between two
    runs of LEN_GUARD canary words.  `out` and `out_len` are what a launch is handed.  Use as a context manager."""

    def __init__(self, ctx, n_utt, stride, pcm16=False, base_offset=0):
        self.ctx, self.n_utt, self.stride, self.pcm16, self.base_offset = ctx, n_utt, int(stride), pcm16, base_offset
        self.item = 2 if pcm16 else 4
        self.dtype = np.uint16 if pcm16 else np.uint32
        self.canary = CANARY16 if pcm16 else CANARY
        assert base_offset in (0, self.item) and GUARD % 8 == 0
        self.rows = n_utt + 2 * GUARD
        self.nbytes = base_offset + self.rows * self.stride * self.item
        self.d_out = self.d_len = None

    def __enter__(self):
        ctx = self.ctx
        self.d_out = ctx.device_alloc(self.nbytes)
        self.d_len = ctx.device_alloc((self.n_utt + 2 * LEN_GUARD) * 4)
        # (filled by a copy of a host array: a memset sets bytes; the words in front of a shifted base are canary halves)
        fill = np.concatenate([np.full(self.base_offset // 2, CANARY16, dtype=np.uint16).view(np.uint8),
                               np.full(self.rows * self.stride, self.canary, dtype=self.dtype).view(np.uint8)])
        assert fill.nbytes == self.nbytes
        ctx.h2d(self.d_out, fill, self.nbytes)
        lens = np.full(self.n_utt + 2 * LEN_GUARD, LEN_CANARY, dtype=np.uint32)
        ctx.h2d(self.d_len, lens, lens.nbytes)
        self.out = C.c_void_p(self.d_out.value + self.base_offset + GUARD * self.stride * self.item)
        self.out_len = C.c_void_p(self.d_len.value + LEN_GUARD * 4)
        return self

    def __exit__(self, *a):
        self.ctx.device_free(self.d_out)
        self.ctx.device_free(self.d_len)

    def download(self):
        """(front: the bytes in front of a shifted base, rows [GUARD + n_utt + GUARD, stride] as uint32 / uint16,
        lens [LEN_GUARD + n_utt + LEN_GUARD])."""
        raw = np.zeros(self.nbytes, dtype=np.uint8)
        self.ctx.d2h(raw, self.d_out, self.nbytes)
        lens = np.zeros(self.n_utt + 2 * LEN_GUARD, dtype=np.uint32)
        self.ctx.d2h(lens, self.d_len, lens.nbytes)
        rows = raw[self.base_offset:].view(self.dtype).reshape(self.rows, self.stride)
        return raw[:self.base_offset], rows, lens


def first_bad(mask):
    """(row, index) of the first True of a 2-d mask, or None."""
    if not mask.any():
        return None
    r = int(np.argmax(mask.any(axis=1)))
    return r, int(np.argmax(mask[r]))


def check_guards(front, rows, lens, n_utt, counts, pcm16, what):
    """Everything a launch may not have touched: the words from every row's count to its stride, the guard rows in front
    and behind, the bytes in front of a shifted base, the words around out_len.  counts[u]: samples row u may hold."""
    canary = CANARY16 if pcm16 else CANARY
    assert np.all(front.view(np.uint16) == CANARY16), f"{what}: the bytes in front of the shifted base were written: {front}"
    for name, block, first in (("in front of the first row", rows[:GUARD], -GUARD), ("behind the last row", rows[GUARD + n_utt:], n_utt)):
        bad = first_bad(block != canary)
        assert bad is None, (f"{what}: guard row {first + bad[0]} ({name}) was written at index {bad[1]}: "
                             f"{int(block[bad]):#x} ({int((block != canary).sum())} words)")
    own = rows[GUARD:GUARD + n_utt]
    past = np.arange(own.shape[1])[None, :] >= np.asarray(counts, dtype=np.int64)[:, None]
    bad = first_bad(past & (own != canary))
    assert bad is None, (f"{what}: row {bad[0]} of {int(counts[bad[0]])} samples was written at index {bad[1]}: "
                         f"{int(own[bad]):#x} ({int((past & (own != canary)).sum())} words past the rows' counts, "
                         f"{int((past & (own != canary))[bad[0]].sum())} of them in this row)")
    for name, g in (("in front of", lens[:LEN_GUARD]), ("behind", lens[LEN_GUARD + n_utt:])):
        assert np.all(g == LEN_CANARY), f"{what}: out_len was written {name} its n_utt words, at {np.flatnonzero(g != LEN_CANARY)[:8]}"


def check_lengths(lens, want, what):
    got = lens[LEN_GUARD:LEN_GUARD + len(want)]
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (f"{what}: out_len differs from the oracle's for {len(bad)} rows, first row {bad[0]}: "
                           f"{int(got[bad[0]])} ({int(got[bad[0]]):#x}) instead of {int(want[bad[0]])}")


def check_bits(own, want, counts, what):
    """own[u, :counts[u]] == want[u, :counts[u]] as bit patterns (uint32 words or uint16 halves)."""
    w = min(own.shape[1], want.shape[1])
    assert int(np.max(counts, initial=0)) <= w
    valid = np.arange(w)[None, :] < np.asarray(counts, dtype=np.int64)[:, None]
    bad = first_bad(valid & (own[:, :w] != want[:, :w]))
    assert bad is None, (f"{what}: row {bad[0]} first differs at sample {bad[1]} of {int(counts[bad[0]])}: {int(own[bad]):#x} "
                         f"instead of {int(want[bad]):#x} ({int((valid & (own[:, :w] != want[:, :w])).sum())} samples differ)")


def check_tolerance(own, ref, counts, what):
    """|x - ref| <= G.FAST_TOLERANCE * max(1, peak(ref)) over every row's samples (own: uint32 words of f32 rows)."""
    w = min(own.shape[1], ref.shape[1])
    valid = np.arange(w)[None, :] < np.asarray(counts, dtype=np.int64)[:, None]
    x = own[:, :w].view(np.float32).astype(np.float64)
    r = np.where(valid, ref[:, :w].astype(np.float64), 0.0)
    peak = np.maximum(1.0, np.abs(r).max(axis=1, initial=0.0))
    with np.errstate(invalid="ignore"):
        d = np.where(valid, np.abs(x - r), 0.0)
    d = np.where(valid & ~np.isfinite(x), np.inf, d)
    bad = first_bad(d > G.FAST_TOLERANCE * peak[:, None])
    assert bad is None, (f"{what}: row {bad[0]} sample {bad[1]} of {int(counts[bad[0]])} is {x[bad]!r} against {r[bad]!r}: "
                         f"{d[bad] / 2.0 ** -23:.1f} * 2^-23 with a peak of {peak[bad[0]]:.3f}")
    return float((d / peak[:, None]).max(initial=0.0))
