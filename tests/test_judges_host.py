"""The on-device judges without a GPU (include/grail_hip.h: grail_batch_digest, grail_batch_compare, grail_pcm16_async).

The numpy models of the three contracts, written from the header's words, that tests/test_judges_gpu.py compares the
device with: digest_model(), compare_model() and pcm16_model(); the corpora both files use (awkward rows, planted single
samples, the non-finite table, every PCM code's truncation boundaries); and, on the CPU, that the models say what the
contract says, that the corpora have the properties the GPU tests assume, and what each judge CANNOT see — so that
nobody relies on either alone."""
import math

import numpy as np

import oracle_lib as O
from test_levels_gpu import _awkward

FLT_MAX = np.float32(3.4028234663852886e38)
NAN, INF = np.float32(np.nan), np.float32(np.inf)
LENGTHS = [0, 1, 255, 256, 257, 511, 512, 513, 4099, 10001]       # one thread, one stride of the workgroup, one more, ragged
BASE_LEN = 1000
PLANTS = [0, 1, 63, 64, 127, 255, 256, 257, 511, 998, 999]        # wave and workgroup-stride boundaries, the last samples
SPECIALS = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-39, 3e38, -3e38, np.nan, np.inf, -np.inf, 1.0], np.float32)
PCM_LENGTHS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4097]             # one lane's 8 samples, one workgroup's 2048, +-1
PCM_ROW = 10000


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def f32_from_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


# ---- the contracts in numpy ------------------------------------------------------------------------------------------
def digest_model(rows, lens):
    """(sums uint64, maxabs float32, nonfinite uint32), one per row: the sum of the uint32 views of the first lens[u]
    samples, the largest finite |x| (0.0 where there is none), the count of NaN and Inf"""
    n = len(lens)
    sums, maxabs, bad = np.zeros(n, np.uint64), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    for u in range(n):
        x = np.ascontiguousarray(rows[u], np.float32)[:int(lens[u])]
        sums[u] = x.view(np.uint32).astype(np.uint64).sum(dtype=np.uint64)
        a = np.abs(x)
        with np.errstate(invalid="ignore"):
            finite = a <= FLT_MAX
        bad[u] = np.count_nonzero(~finite)
        maxabs[u] = a[finite].max() if finite.any() else np.float32(0.0)
    return sums, maxabs, bad


def compare_model(a, b, len_a, len_b):
    """(maxdiff float32, sumsq float64, mismatches uint32), one per row, over the first len_a[u] samples: d = |a - b| in
    binary32 (the subtraction rounds, and may overflow); a finite d enters maxdiff, and float64(d)^2 (exact) enters sumsq,
    here the correctly rounded sum (math.fsum); a d that is not finite is a mismatch unless the bit patterns are equal or
    both sides are NaN; one more mismatch where the lengths differ"""
    n = len(len_a)
    maxdiff, sumsq, bad = np.zeros(n, np.float32), np.zeros(n, np.float64), np.zeros(n, np.uint32)
    for u in range(n):
        k = int(len_a[u])
        x, y = np.ascontiguousarray(a[u], np.float32)[:k], np.ascontiguousarray(b[u], np.float32)[:k]
        with np.errstate(all="ignore"):
            d = np.abs(x - y)
            finite = d <= FLT_MAX
        assert d.dtype == np.float32
        d64 = d[finite].astype(np.float64)
        maxdiff[u] = d[finite].max() if finite.any() else np.float32(0.0)
        sumsq[u] = math.fsum((d64 * d64).tolist())
        equal = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        bad[u] = np.count_nonzero(~finite & ~equal) + (1 if int(len_a[u]) != int(len_b[u]) else 0)
    return maxdiff, sumsq, bad


def pcm16_model(x):
    """`(x * i16::MAX as f32) as i16`: a binary32 multiply by 32767.0f, truncation toward zero, a clamp to
    [-32768, 32767], NaN -> 0"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        y = x * np.float32(32767.0)
        assert y.dtype == np.float32
        t = np.clip(np.trunc(y), np.float32(-32768.0), np.float32(32767.0))
    return np.where(np.isnan(y), np.float32(0.0), t).astype(np.int16)


# ---- the corpora -----------------------------------------------------------------------------------------------------
def judge_rows():
    """rows of LENGTHS with -0.0, denormals, 3e38, NaN and +-Inf sprinkled in, a row of uniformly random 32-bit patterns,
    a row that is all NaN (three payloads) or Inf, and a row of -0.0"""
    rng = np.random.default_rng(101)
    rows = [_awkward(rng, n) for n in LENGTHS]
    rows[1][0] = np.float32(-0.5)
    for x in rows[2:]:                                           # a row's last sample is one a skipped tail would miss
        x[-1] = np.float32(0.3125)
    rows.append(rng.integers(0, 2 ** 32, 3001, dtype=np.uint64).astype(np.uint32).view(np.float32))
    nonfinite = np.array([0x7FC00000, 0xFFFFFFFF, 0x7F800001, 0x7F800000, 0xFF800000], np.uint32).view(np.float32)
    rows.append(nonfinite[rng.integers(0, len(nonfinite), 777)])
    rows.append(np.full(600, -0.0, np.float32))
    return rows


def noisy_copy(rows, seed=102):
    """every sample's bit pattern moved by -3 ... 3 (a few units in the last place; a zero, an infinity or a NaN becomes
    whatever that gives), about one sample in forty replaced from SPECIALS, and a row's last sample one unit above"""
    rng = np.random.default_rng(seed)
    out = []
    for x in rows:
        y = (_bits(x) + rng.integers(-3, 4, len(x)).astype(np.uint32)).view(np.float32).copy()
        mask = rng.random(len(x)) < 1.0 / 40.0
        y[mask] = SPECIALS[rng.integers(0, len(SPECIALS), int(mask.sum()))]
        if len(x) > 1:                                           # the last sample always differs: a skipped tail is seen
            y[-1:] = (_bits(x[-1:]) + np.uint32(1)).view(np.float32)
        out.append(y)
    return out


def base_row():
    """1000 finite samples of audio size, none of them zero; one +0.0 at 500 (for the sign-of-zero cases)"""
    x = (np.random.default_rng(103).standard_normal(BASE_LEN) * 0.2).astype(np.float32)
    x[x == 0] = np.float32(0.1)
    assert 500 not in PLANTS
    x[500] = np.float32(0.0)
    return x


def planted_digest_rows():
    """(base, flipped, nans): copy k of the base row with the low mantissa bit of sample PLANTS[k] flipped, and with that
    sample made NaN"""
    base = base_row()
    flipped, nans = [], []
    for p in PLANTS:
        r = base.copy()
        r.view(np.uint32)[p] ^= 1
        flipped.append(r)
        r = base.copy()
        r[p] = NAN
        nans.append(r)
    return base, flipped, nans


def planted_compare_rows():
    """(a, b) of 2 x 11 + 4 rows of BASE_LEN + 1 samples (the last one lies past the length):
    0 ... 10    b's sample PLANTS[k] one unit in the last place above a's
    11 ... 21   a's sample PLANTS[k] 0.0, b's 1e-45 (the smallest denormal)
    22          nothing planted
    23          a's +0.0 at 500 is -0.0 in b
    24          the only difference at index BASE_LEN, just past the length
    25          b is a permutation of a (its first and last samples swapped)"""
    base = np.concatenate([base_row(), np.array([0.375], np.float32)])
    a, b = [], []
    for p in PLANTS:
        a.append(base.copy())
        b.append(base.copy())
        b[-1][p] = np.nextafter(base[p], INF)
    for p in PLANTS:
        a.append(base.copy())
        b.append(base.copy())
        a[-1][p], b[-1][p] = np.float32(0.0), np.float32(1e-45)
    for _ in range(4):
        a.append(base.copy())
        b.append(base.copy())
    b[23][500] = np.float32(-0.0)
    b[24][BASE_LEN] = np.float32(-0.375)
    b[25][0], b[25][BASE_LEN - 1] = base[BASE_LEN - 1], base[0]
    return a, b


NONFINITE_TABLE = [                     # (a, b, mismatches); none of them enters maxdiff or sumsq
    (f32_from_bits(0x7FC00000), f32_from_bits(0xFFC00123), 0),   # NaN against NaN, different payloads and signs
    (INF, INF, 0),
    (-INF, -INF, 0),
    (INF, -INF, 1),
    (NAN, INF, 1),
    (NAN, np.float32(1.0), 1),
    (np.float32(1.0), -INF, 1),
    (np.float32(3e38), np.float32(-3e38), 1),                    # both finite, the difference overflows
]
TABLE_LEN = 700


def nonfinite_table_rows():
    """(a, b, mismatches): one row of TABLE_LEN samples per pair of NONFINITE_TABLE, the pair at sample 250 + 37 k (every
    stride of the workgroup, several lanes); a last row holds rows 3, 5 and 7's pairs and row 0's (3 mismatches).  The
    rest of each row is equal and finite, but for 0.25 against 0.5 at the last sample: maxdiff 0.25, sumsq 0.0625"""
    rest = (np.random.default_rng(104).standard_normal(TABLE_LEN) * 0.2).astype(np.float32)
    a, b, want = [], [], []
    for k, (x, y, m) in enumerate(NONFINITE_TABLE):
        a.append(rest.copy())
        b.append(rest.copy())
        a[-1][250 + 37 * k], b[-1][250 + 37 * k] = x, y
        want.append(m)
    a.append(rest.copy())
    b.append(rest.copy())
    for p, k in ((3, 3), (256, 5), (698, 7), (511, 0)):
        a[-1][p], b[-1][p] = NONFINITE_TABLE[k][0], NONFINITE_TABLE[k][1]
    want.append(3)
    for x, y in zip(a, b):
        x[-1], y[-1] = np.float32(0.25), np.float32(0.5)
    return a, b, np.array(want, np.uint32)


def pcm16_boundary_values():
    """for every integer k of -32768 ... 32768 the binary32 value nearest k / 32767, the one below and the one above it
    (the conversion truncates: the code changes at k / 32767), and the values at the ends of the range"""
    v = (np.arange(-32768, 32769, dtype=np.float64) / 32767.0).astype(np.float32)
    ends = np.array([0.0, 1e-45, 1.0, 1.0 + 2.0 ** -23, 2.0, 3e38, np.inf], np.float32)
    return np.concatenate([v, np.nextafter(v, -INF), np.nextafter(v, INF), ends, -ends, np.array([np.nan], np.float32)])


def pcm16_rows():
    """the boundary values in a fixed random order as rows of PCM_LENGTHS, then rows of PCM_ROW (the last one filled up
    with audio-sized noise)"""
    rng = np.random.default_rng(105)
    v = pcm16_boundary_values()
    v = v[rng.permutation(len(v))]
    n_long = -(-(len(v) - sum(PCM_LENGTHS)) // PCM_ROW)
    lens = PCM_LENGTHS + [PCM_ROW] * n_long
    v = np.concatenate([v, (rng.standard_normal(sum(lens) - len(v)) * 0.6).astype(np.float32)])
    ends = np.cumsum(lens)
    return [v[e - n:e] for e, n in zip(ends, lens)]


# ---- the models say what the contract says ---------------------------------------------------------------------------
def test_pcm16_model_equals_the_oracle_on_every_boundary():
    v = pcm16_boundary_values()
    assert len(v) == 3 * 65537 + 15 and np.isnan(v[-1])
    L = O.lib()
    want = np.array([L.orc_pcm16(float(x)) for x in v], np.int16)
    got = pcm16_model(v)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert set(got.tolist()) == set(range(-32768, 32768))       # every code is produced
    # the set aims at the boundaries: rounding to nearest instead of truncating would move a third of it
    with np.errstate(all="ignore"):
        y = (v * np.float32(32767.0))[np.isfinite(v) & (np.abs(v) < 1)]
    assert np.count_nonzero(np.rint(y) != np.trunc(y)) > 60000


def test_pcm16_rows_hold_every_boundary_value():
    rows = pcm16_rows()
    assert [len(r) for r in rows[:len(PCM_LENGTHS)]] == PCM_LENGTHS and all(len(r) == PCM_ROW for r in rows[len(PCM_LENGTHS):])
    v = pcm16_boundary_values()
    allv = np.concatenate(rows)
    assert len(allv) >= len(v) and len(allv) - len(v) < PCM_ROW
    assert np.array_equal(np.sort(_bits(allv[:len(v)])), np.sort(_bits(v)))


def test_digest_model_on_values_known_by_hand():
    rows = [np.array([1.0, -2.0, np.nan, np.inf, -0.0, 9.0], np.float32), np.array([np.nan, -np.inf], np.float32),
            np.zeros(4, np.float32)]
    sums, maxabs, bad = digest_model(rows, [5, 2, 0])
    assert sums.tolist() == [0x3F800000 + 0xC0000000 + 0x7FC00000 + 0x7F800000 + 0x80000000, 0x7FC00000 + 0xFF800000, 0]
    assert maxabs.tolist() == [2.0, 0.0, 0.0] and bad.tolist() == [2, 2, 0]


def test_compare_model_subtracts_in_binary32_and_keeps_denormals():
    a = [np.array([0.0, 1.0, 16777216.0], np.float32)]
    b = [np.array([1e-45, 1.0, -1.0], np.float32)]
    maxdiff, sumsq, bad = compare_model(a, b, [1], [1])
    assert maxdiff[0] == np.float32(1e-45) and maxdiff[0] > 0 and sumsq[0] == float(np.float32(1e-45)) ** 2 > 0 and bad[0] == 0
    maxdiff, sumsq, bad = compare_model(a, b, [3], [2])
    assert maxdiff[0] == np.float32(16777216.0) and bad[0] == 1  # 2^24 + 1 rounds to 2^24 in binary32; the lengths differ


def test_compare_model_on_the_non_finite_table():
    a, b, want = nonfinite_table_rows()
    lens = [TABLE_LEN] * len(a)
    for x, y in ((a, b), (b, a)):
        maxdiff, sumsq, bad = compare_model(x, y, lens, lens)
        assert np.array_equal(bad, want), bad
        assert np.all(maxdiff == np.float32(0.25)) and np.all(sumsq == 0.0625)
    assert want.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 3]
    # without the finite pair at the end nothing at all enters maxdiff or sumsq
    maxdiff, sumsq, bad = compare_model(a, b, [TABLE_LEN - 1] * len(a), [TABLE_LEN - 1] * len(a))
    assert np.array_equal(bad, want) and not maxdiff.any() and not sumsq.any()


# ---- what each judge cannot see --------------------------------------------------------------------------------------
def test_the_digest_is_blind_to_a_permutation_and_compare_is_not():
    a, b = planted_compare_rows()
    x, y = a[25][:BASE_LEN], b[25][:BASE_LEN]
    assert not np.array_equal(_bits(x), _bits(y)) and np.array_equal(np.sort(_bits(x)), np.sort(_bits(y)))
    sums, maxabs, bad = digest_model([x, y], [BASE_LEN] * 2)
    assert sums[0] == sums[1] and maxabs[0] == maxabs[1] and bad[0] == bad[1]
    maxdiff, sumsq, _ = compare_model([x], [y], [BASE_LEN], [BASE_LEN])
    assert maxdiff[0] > 0 and sumsq[0] > 0
    rng = np.random.default_rng(1)
    for row in judge_rows():
        assert digest_model([row], [len(row)])[0][0] == digest_model([row[rng.permutation(len(row))]], [len(row)])[0][0]


def test_compare_is_blind_to_the_sign_of_zero_and_the_digest_is_not():
    a, b = planted_compare_rows()
    x, y = a[23][:BASE_LEN], b[23][:BASE_LEN]
    assert np.count_nonzero(_bits(x) != _bits(y)) == 1 and _bits(x)[500] == 0 and _bits(y)[500] == 0x80000000
    maxdiff, sumsq, bad = compare_model([x], [y], [BASE_LEN], [BASE_LEN])
    assert (maxdiff[0], sumsq[0], bad[0]) == (0.0, 0.0, 0)
    sums = digest_model([x, y], [BASE_LEN] * 2)[0]
    assert int(sums[1]) - int(sums[0]) == 0x80000000
    # ... and two opposite flips inside one row are what the two judges together still leave open
    z, w = x.copy(), x.copy()
    z[0], z[500] = np.float32(0.0), np.float32(-0.0)
    w[0], w[500] = np.float32(-0.0), np.float32(0.0)
    sums = digest_model([z, w], [BASE_LEN] * 2)[0]
    assert sums[0] == sums[1] and not np.array_equal(_bits(z), _bits(w))
    maxdiff, sumsq, bad = compare_model([z], [w], [BASE_LEN], [BASE_LEN])
    assert (maxdiff[0], sumsq[0], bad[0]) == (0.0, 0.0, 0)


# ---- the corpora have the properties the GPU tests assume ------------------------------------------------------------
def test_awkward_rows_hold_what_they_are_meant_to():
    rows = judge_rows()
    assert [len(r) for r in rows[:len(LENGTHS)]] == LENGTHS and max(len(r) for r in rows) == 10001
    sums, maxabs, bad = digest_model(rows, [len(r) for r in rows])
    assert bad[:len(LENGTHS)].sum() > 20 and maxabs[9] == np.float32(3e38)
    assert maxabs[-2] == 0.0 and bad[-2] == len(rows[-2])        # all NaN or Inf
    assert sums[-1] == 600 * 0x80000000 and maxabs[-1] == 0.0 and bad[-1] == 0
    for r in rows[2:]:                                           # a skipped tail, or a thread started a stride late, is seen
        assert _bits(r)[-1] != 0 and np.count_nonzero(_bits(r)[:256]) > 0
    b = noisy_copy(rows)
    lens = [len(r) for r in rows]
    maxdiff, sumsq, mism = compare_model(rows, b, lens, lens)
    assert mism.sum() > 100 and np.all(maxdiff[2:len(LENGTHS) + 1] > 0) and np.isfinite(sumsq).all()
    # ... also in each row's tail after its last full stride of 256, and in its first stride
    for x, y in zip(rows[2:len(LENGTHS)], b[2:len(LENGTHS)]):
        n = len(x)
        if n % 256:
            assert compare_model([x[n & ~255:]], [y[n & ~255:]], [n % 256], [n % 256])[1][0] > 0
        assert compare_model([x[:256]], [y[:256]], [min(n, 256)], [min(n, 256)])[1][0] > 0


def test_planted_rows_differ_from_their_base_inside_their_length():
    assert max(PLANTS) == BASE_LEN - 1 and min(PLANTS) == 0 and len(PLANTS) == 11
    base, flipped, nans = planted_digest_rows()
    assert len(base) == BASE_LEN and np.isfinite(base).all()
    s0 = int(digest_model([base], [BASE_LEN])[0][0])
    for rows, nonfinite in ((flipped, 0), (nans, 1)):
        sums, _, bad = digest_model(rows, [BASE_LEN] * len(rows))
        assert np.all(bad == nonfinite) and len(rows) == len(PLANTS)
        for k, p in enumerate(PLANTS):
            changed = np.nonzero(_bits(rows[k]) != _bits(base))[0]
            assert changed.tolist() == [p] and int(sums[k]) != s0
    for k, p in enumerate(PLANTS):
        assert abs(int(digest_model([flipped[k]], [BASE_LEN])[0][0]) - s0) == 1
    a, b = planted_compare_rows()
    assert len(a) == 26 and all(len(r) == BASE_LEN + 1 for r in a + b)
    lens = [BASE_LEN] * len(a)
    maxdiff, sumsq, bad = compare_model(a, b, lens, lens)
    assert not bad.any()
    for k in range(22):
        changed = np.nonzero(_bits(a[k]) != _bits(b[k]))[0]
        assert changed.tolist() == [PLANTS[k % 11]] and maxdiff[k] > 0 and sumsq[k] > 0
    assert np.all(maxdiff[11:22] == np.float32(1e-45))
    assert not maxdiff[22:25].any() and not sumsq[22:25].any() and maxdiff[25] > 0
    assert np.nonzero(_bits(a[24]) != _bits(b[24]))[0].tolist() == [BASE_LEN]
