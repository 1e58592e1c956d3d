"""The on-device judges themselves (csrc/pcm_kernels.hip): grail_batch_digest and grail_batch_compare — on whose word every
full-size claim of this suite rests — and grail_pcm16_async, each against its numpy model (tests/test_judges_host.py:
digest_model, compare_model, pcm16_model) on rows of every awkward length and value, under every layout of the same rows,
among other rows, and on rows that differ from a base row in ONE planted sample: a judge that skipped a row's tail,
started a stride late or returned zeros fails here.  Every case is one or two launches on rows of at most 10 001 samples.

Neither digest nor compare clamps a length to the stride: no case here has a length above it."""
import ctypes as C

import numpy as np
import pytest

import grail_hip as G
from test_judges_host import (BASE_LEN, INF, LENGTHS, NAN, PLANTS, TABLE_LEN, _bits, base_row, compare_model, digest_model,
                              judge_rows, noisy_copy, nonfinite_table_rows, pcm16_model, pcm16_rows, planted_compare_rows,
                              planted_digest_rows)
from test_levels_gpu import CANARY, Dev, dev, same_bits  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
LONGEST = max(LENGTHS)
LAYOUTS = {"stride64": ((LONGEST + 63) // 64 * 64, 0, 0), "odd": (LONGEST + 2, 0, 0), "offset1": ((LONGEST + 63) // 64 * 64, 1, 1),
           "offset3": ((LONGEST + 63) // 64 * 64, 3, 3), "offsets1and2": ((LONGEST + 63) // 64 * 64, 1, 2)}
ROW_STRIDE = 1024                                                 # of the planted rows (BASE_LEN + 1 samples at most)


@pytest.fixture(scope="module")
def judged():
    """the awkward rows, their noisy copies, and what the models say of them"""
    rows = judge_rows()
    lens = np.array([len(r) for r in rows], np.uint32)
    b = noisy_copy(rows)
    return dict(rows=rows, lens=lens, digest=digest_model(rows, lens), b=b, compare=compare_model(rows, b, lens, lens))


def _lay(dev, rows, lens, stride, offset=0, fill=CANARY, positions=None, other_lens=None):
    """rows[i] (which may hold samples past lens[i]) as row positions[i] of a device buffer of len(other_lens) rows at
    `stride`, `offset` floats past an allocation's (256-byte aligned) start.  Everything else holds `fill`: the floats in
    front of the base, a guard row before the first row and one after the last, every gap up to the stride, the other
    rows.  -> (rows_dev, all the rows' lengths)"""
    all_lens = np.zeros(len(rows), np.uint32) if other_lens is None else np.array(other_lens, np.uint32)
    positions = range(len(rows)) if positions is None else positions
    host = np.full(offset + (len(all_lens) + 2) * stride, fill, np.float32)
    for x, n, p in zip(rows, lens, positions):
        assert n <= len(x) <= stride and n <= stride, "no length above the stride: the judges do not clamp it"
        at = offset + (p + 1) * stride
        host[at:at + len(x)] = x
        all_lens[p] = n
    base = dev.up(host)
    return C.c_void_p(base.value + (offset + stride) * 4), all_lens


def _same(got, want, what):
    """exact (floats: bit for bit), with the first row that differs in the message"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    miss = np.nonzero(got.view(u) != want.view(u))[0]
    assert len(miss) == 0, f"{what}: {len(miss)} rows differ, first row {miss[0]}: got {got[miss[0]]!r}, want {want[miss[0]]!r}"


def _same_sumsq(got, want, lens, what):
    """n * 2^-52 relative to the correctly rounded sum: the bound for n - 1 binary64 additions of non-negative terms in
    ANY order (each term, the square of a binary32 value, is exact in binary64) — the order of summation is not pinned"""
    for u in range(len(want)):
        print(f"{what}: row {u} of {lens[u]} samples, sumsq {got[u]!r} against {want[u]!r}")
        assert abs(got[u] - want[u]) <= int(lens[u]) * 2.0 ** -52 * want[u], (what, u, got[u], want[u])


# ---- digest ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["3e38", "nan"])
@pytest.mark.parametrize("layout", ["stride64", "odd", "offset1", "offset3"])
def test_digest_equals_the_model(gpu_ctx, dev, judged, layout, fill):
    """rows of 0 ... 10 001 samples with every awkward value, a row of random bit patterns, a row that is all NaN or Inf, a
    row of -0.0: sums and nonfinite exact, maxabs bit for bit — at a stride that is a multiple of 64, at an odd one, and
    with the base 1 and 3 floats past an aligned address; everything outside the rows' samples holds 3e38, or NaN, so a
    read one sample too far shows in all three numbers"""
    stride, offset, _ = LAYOUTS[layout]
    assert stride % 2 == (1 if layout == "odd" else 0) and stride > LONGEST
    rows_dev, lens = _lay(dev, judged["rows"], judged["lens"], stride, offset, {"3e38": np.float32(3e38), "nan": NAN}[fill])
    sums, maxabs, bad = gpu_ctx.digest(rows_dev, stride, dev.up(lens), len(lens))
    ws, wm, wb = judged["digest"]
    _same(sums, ws, f"sums, {layout}, {fill} outside")
    _same(bad, wb, f"nonfinite, {layout}, {fill} outside")
    _same(maxabs, wm, f"maxabs, {layout}, {fill} outside")
    assert maxabs[-2] == 0.0 and bad[-2] == lens[-2] and sums[0] == 0 and sums[-1] == int(lens[-1]) * 0x80000000


def test_digest_sees_every_planted_sample(gpu_ctx, dev):
    """one base row of 1000 samples and 2 x 11 copies in one launch, copy k with the low mantissa bit of sample p_k flipped
    (p = 0, 1, 63, 64, 127, 255, 256, 257, 511, 998, 999), and with that sample NaN: every copy's sum differs from the base
    row's by exactly the model's amount, nonfinite is 0 and 1; a copy changed only at index 1000, just past the length,
    gives the base row's numbers"""
    base, flipped, nans = planted_digest_rows()
    past = np.concatenate([base, np.array([7.0], np.float32)])
    rows = [base] + flipped + nans + [past]
    lens = [BASE_LEN] * len(rows)
    ws, wm, wb = digest_model(rows, lens)
    for offset in (0, 1):
        rows_dev, all_lens = _lay(dev, rows, lens, ROW_STRIDE, offset)
        sums, maxabs, bad = gpu_ctx.digest(rows_dev, ROW_STRIDE, dev.up(all_lens), len(rows))
        for k in range(1, 23):
            moved, want = int(sums[k]) - int(sums[0]), int(ws[k]) - int(ws[0])
            assert moved == want != 0, f"sample {PLANTS[(k - 1) % 11]} of row {k}: the sum moved by {moved}, the model's by {want}"
        _same(sums, ws, "sums")
        _same(bad, np.array([0] + [0] * 11 + [1] * 11 + [0], np.uint32), "nonfinite")
        _same(maxabs, wm, "maxabs")
        assert (sums[-1], maxabs[-1], bad[-1]) == (sums[0], maxabs[0], bad[0]), "a sample past the length was read"


@pytest.mark.parametrize("n_rows", [1, 257, 300])
def test_digest_of_a_row_does_not_depend_on_the_rows_around_it(gpu_ctx, dev, n_rows):
    """the base row at a random position among 1, 257 and 300 rows: the same three numbers; the other rows (3e38 over a
    random length up to the stride) theirs"""
    rng = np.random.default_rng(n_rows)
    base = base_row()
    pos = int(rng.integers(0, n_rows))
    other = rng.integers(0, ROW_STRIDE + 1, n_rows)
    rows_dev, lens = _lay(dev, [base], [BASE_LEN], ROW_STRIDE, 0, np.float32(3e38), [pos], other)
    sums, maxabs, bad = gpu_ctx.digest(rows_dev, ROW_STRIDE, dev.up(lens), n_rows)
    ws, wm, wb = digest_model([base], [BASE_LEN])
    assert (sums[pos], bad[pos]) == (ws[0], wb[0]) and same_bits(maxabs[pos:pos + 1], wm), (pos, sums[pos], maxabs[pos], bad[pos])
    rest = np.setdiff1d(np.arange(n_rows), [pos])
    _same(sums[rest], lens[rest].astype(np.uint64) * np.uint64(_bits(np.float32(3e38))[0]), "the other rows' sums")
    _same(maxabs[rest], np.where(lens[rest] > 0, np.float32(3e38), np.float32(0.0)).astype(np.float32), "the other rows' maxabs")
    assert not bad[rest].any()


def test_digest_arguments(gpu_ctx, dev):
    lib = G.load()
    assert lib.grail_batch_digest(gpu_ctx.handle, None, 0, None, 0, None, None, None) == G.OK
    d_rows, d_len = dev.up(np.zeros(128, np.float32)), dev.up(np.array([64], np.uint32))
    for rows, lens in ((None, d_len), (d_rows, None)):
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.digest(rows, 64, lens, 1)
        assert ei.value.status == G.ERR_INVALID_ARG
    sums, maxabs, bad = gpu_ctx.digest(d_rows, 64, d_len, 1)
    assert (sums[0], maxabs[0], bad[0]) == (0, 0.0, 0)


# ---- compare ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["3e38|nan", "0.5|-0.5"])
@pytest.mark.parametrize("layout", ["stride64", "odd", "offset1", "offset3", "offsets1and2"])
def test_compare_equals_the_model(gpu_ctx, dev, judged, layout, fill):
    """a = the digest test's rows, b = a with every sample moved by a few units in the last place and one in forty
    replaced by -0.0, a denormal, 3e38, NaN, +-Inf ...: maxdiff bit for bit, mismatches exact, sumsq within n * 2^-52 of
    the correctly rounded sum; the same numbers with the arguments swapped (the lengths agree).  Outside the rows' samples
    a holds 3e38 and b NaN (a read too far is a mismatch), or 0.5 and -0.5 (it enters maxdiff and sumsq)"""
    stride, off_a, off_b = LAYOUTS[layout]
    fa, fb = {"3e38|nan": (np.float32(3e38), NAN), "0.5|-0.5": (np.float32(0.5), np.float32(-0.5))}[fill]
    a_dev, lens = _lay(dev, judged["rows"], judged["lens"], stride, off_a, fa)
    b_dev, _ = _lay(dev, judged["b"], judged["lens"], stride, off_b, fb)
    d_len = dev.up(lens)
    maxdiff, sumsq, bad = gpu_ctx.compare(a_dev, b_dev, stride, d_len, d_len, len(lens))
    wm, wq, wb = judged["compare"]
    what = f"{layout}, {fill} outside"
    _same(bad, wb, "mismatches, " + what)
    _same(maxdiff, wm, "maxdiff, " + what)
    _same_sumsq(sumsq, wq, lens, what)
    assert bad.sum() > 100 and (maxdiff[0], sumsq[0], bad[0]) == (0.0, 0.0, 0)
    maxdiff2, sumsq2, bad2 = gpu_ctx.compare(b_dev, a_dev, stride, d_len, d_len, len(lens))
    _same(bad2, bad, "mismatches, swapped")
    _same(maxdiff2, maxdiff, "maxdiff, swapped")
    _same(sumsq2, sumsq, "sumsq, swapped")


def test_compare_sees_every_planted_difference_and_nothing_else(gpu_ctx, dev):
    """a = 26 copies of a base row of 1000 samples; b differs in ONE sample a row, at p = 0, 1, 63, 64, 127, 255, 256, 257, 511,
    998, 999: by one unit in the last place, and 0.0 against 1e-45 (which must come back as 1.4e-45, not flushed to
    zero): exactly the model's maxdiff, sumsq = maxdiff^2 > 0.  A row with nothing planted, one whose only difference is
    -0.0 against +0.0, and one whose only difference lies at index len_a report exactly (0.0, 0.0, 0).
    And the two judges together: the row that is a permutation of its partner has its digest and a compare > 0; the row
    with the zero's sign flipped compares equal and has another digest"""
    a, b = planted_compare_rows()
    lens = [BASE_LEN] * len(a)
    wm, wq, wb = compare_model(a, b, lens, lens)
    for off_a, off_b in ((0, 0), (1, 3)):
        a_dev, all_lens = _lay(dev, a, lens, ROW_STRIDE, off_a)
        b_dev, _ = _lay(dev, b, lens, ROW_STRIDE, off_b)
        d_len = dev.up(all_lens)
        maxdiff, sumsq, bad = gpu_ctx.compare(a_dev, b_dev, ROW_STRIDE, d_len, d_len, len(a))
        for k in range(22):
            p = PLANTS[k % 11]
            want = np.float32(1e-45) if k >= 11 else np.nextafter(a[k][p], INF) - a[k][p]
            assert want > 0 and same_bits(maxdiff[k:k + 1], np.array([want], np.float32)), \
                f"row {k}, the difference at sample {p}: maxdiff {maxdiff[k]!r}, planted {want!r}"
            assert sumsq[k] == float(want) ** 2 > 0, (k, p, sumsq[k], float(want) ** 2)
        _same(maxdiff, wm, "maxdiff")
        _same(sumsq, wq, "sumsq (one term a row: exact)")
        _same(bad, wb, "mismatches")
        for k, why in ((22, "nothing planted"), (23, "-0.0 against +0.0"), (24, "a difference at index len_a")):
            assert same_bits(maxdiff[k:k + 1], np.zeros(1, np.float32)) and same_bits(sumsq[k:k + 1], np.zeros(1)) \
                and bad[k] == 0, (why, maxdiff[k], sumsq[k], bad[k])
        assert maxdiff[25] > 0 and sumsq[25] > 0 and not bad.any()
        sums_a, maxabs_a, bad_a = gpu_ctx.digest(a_dev, ROW_STRIDE, d_len, len(a))
        sums_b, maxabs_b, bad_b = gpu_ctx.digest(b_dev, ROW_STRIDE, d_len, len(a))
        assert sums_a[25] == sums_b[25] and maxabs_a[25] == maxabs_b[25]          # blind to the permutation
        assert int(sums_b[23]) - int(sums_a[23]) == 0x80000000                    # not to the sign of the zero
        assert sums_a[22] == sums_b[22] and sums_a[24] == sums_b[24]
        assert np.all(sums_a[:22] != sums_b[:22])


def test_compare_at_the_edge_of_the_fast_tolerance(gpu_ctx, dev):
    """the comparison every caller makes, maxdiff <= GRAIL_FAST_TOLERANCE: it holds for rows whose one difference is
    exactly the tolerance (0.0 against tol, 0.5 against 0.5 + tol: both representable) and fails one binary32 step above"""
    tol = np.float32(G.FAST_TOLERANCE)
    assert float(tol) == G.FAST_TOLERANCE and np.float32(0.5) + tol - np.float32(0.5) == tol
    above = [np.nextafter(tol, INF), np.nextafter(np.float32(0.5) + tol, INF)]
    assert above[0] > tol and above[1] - np.float32(0.5) > tol
    pairs = [(np.float32(0.0), tol), (np.float32(0.5), np.float32(0.5) + tol), (np.float32(0.0), above[0]), (np.float32(0.5), above[1])]
    rest = base_row()[:TABLE_LEN]
    a, b = [], []
    for k, (x, y) in enumerate(pairs):
        a.append(rest.copy())
        b.append(rest.copy())
        a[-1][650 + k], b[-1][650 + k] = x, y
    lens = [TABLE_LEN] * 4
    a_dev, all_lens = _lay(dev, a, lens, ROW_STRIDE)
    b_dev, _ = _lay(dev, b, lens, ROW_STRIDE)
    d_len = dev.up(all_lens)
    maxdiff, sumsq, bad = gpu_ctx.compare(a_dev, b_dev, ROW_STRIDE, d_len, d_len, 4)
    print(f"\nmaxdiff / 2^-23: {(maxdiff.astype(np.float64) * 2.0 ** 23).tolist()}, the tolerance {G.FAST_TOLERANCE * 2.0 ** 23}")
    _same(maxdiff, compare_model(a, b, lens, lens)[0], "maxdiff")
    assert maxdiff[0] == tol and maxdiff[1] == tol and not bad.any()
    assert maxdiff[:2].max() <= G.FAST_TOLERANCE
    assert not maxdiff[2] <= G.FAST_TOLERANCE and not maxdiff[3] <= G.FAST_TOLERANCE
    assert not maxdiff.max() <= G.FAST_TOLERANCE


def test_compare_non_finite_table(gpu_ctx, dev):
    """the header's table, a row a pair: (NaN, NaN) of different payloads, (+Inf, +Inf), (-Inf, -Inf): no mismatch;
    (+Inf, -Inf), (NaN, +Inf), (NaN, 1.0), (1.0, -Inf) and (3e38, -3e38), whose difference overflows: one each; none of them
    enters maxdiff or sumsq, which are exactly those of the remaining samples (0.25 and 0.0625); a row with three such
    samples reports 3; either way round"""
    a, b, want = nonfinite_table_rows()
    lens = [TABLE_LEN] * len(a)
    a_dev, all_lens = _lay(dev, a, lens, ROW_STRIDE)
    b_dev, _ = _lay(dev, b, lens, ROW_STRIDE)
    d_len = dev.up(all_lens)
    for x, y, hx, hy in ((a_dev, b_dev, a, b), (b_dev, a_dev, b, a)):
        maxdiff, sumsq, bad = gpu_ctx.compare(x, y, ROW_STRIDE, d_len, d_len, len(a))
        _same(bad, want, "mismatches")
        _same(maxdiff, np.full(len(a), 0.25, np.float32), "maxdiff")
        _same(sumsq, np.full(len(a), 0.0625), "sumsq")
        wm, wq, wb = compare_model(hx, hy, lens, lens)
        _same(bad, wb, "mismatches against the model")
        _same(maxdiff, wm, "maxdiff against the model")
        _same(sumsq, wq, "sumsq against the model")
    # without the finite pair at the rows' last sample: nothing enters maxdiff or sumsq
    all_lens[:] = TABLE_LEN - 1
    d_len = dev.up(all_lens)
    maxdiff, sumsq, bad = gpu_ctx.compare(a_dev, b_dev, ROW_STRIDE, d_len, d_len, len(a))
    _same(bad, want, "mismatches")
    assert same_bits(maxdiff, np.zeros(len(a), np.float32)) and same_bits(sumsq, np.zeros(len(a)))


def test_compare_lengths(gpu_ctx, dev):
    """len_b = len_a + 1 and len_a - 1 each add exactly 1 and the rows are still compared over len_a samples (the one
    difference is a's last sample; past len_a a holds 3e38 and b finite values); len_a = len_b = 0 gives (0, 0, 0)"""
    n = TABLE_LEN
    rest = base_row()[:n]
    a = [rest.copy() for _ in range(4)]
    b = [np.concatenate([rest, np.full(16, 0.125, np.float32)]) for _ in range(4)]
    for y in b:
        y[n - 1] = rest[n - 1] + np.float32(0.5)
    len_a, len_b = np.array([n, n, 0, n], np.uint32), np.array([n + 1, n - 1, 0, n], np.uint32)
    a_dev, _ = _lay(dev, a, len_a, ROW_STRIDE, 0, np.float32(3e38))
    b_dev, _ = _lay(dev, b, len_b, ROW_STRIDE, 0, np.float32(0.125))
    maxdiff, sumsq, bad = gpu_ctx.compare(a_dev, b_dev, ROW_STRIDE, dev.up(len_a), dev.up(len_b), 4)
    wm, wq, wb = compare_model(a, b, len_a, len_b)
    _same(bad, wb, "mismatches")
    _same(maxdiff, wm, "maxdiff")
    _same(sumsq, wq, "sumsq (one term a row: exact)")
    assert bad.tolist() == [1, 1, 0, 0]
    d = np.abs(rest[n - 1] - b[0][n - 1])
    assert d > 0.4 and maxdiff.tolist() == [d, d, 0.0, d] and sumsq.tolist() == [float(d) ** 2, float(d) ** 2, 0.0, float(d) ** 2]


@pytest.mark.parametrize("n_rows", [1, 257, 300])
def test_compare_of_a_row_does_not_depend_on_the_rows_around_it(gpu_ctx, dev, n_rows):
    """a planted pair (0.0 against 1e-45 at the row's last sample) at a random position among 1, 257 and 300 rows: the same
    numbers; the other rows, equal over a random length up to the stride, (0.0, 0.0, 0)"""
    rng = np.random.default_rng(1000 + n_rows)
    a, b = planted_compare_rows()
    pos = int(rng.integers(0, n_rows))
    other = rng.integers(0, ROW_STRIDE + 1, n_rows)
    a_dev, lens = _lay(dev, [a[21]], [BASE_LEN], ROW_STRIDE, 0, CANARY, [pos], other)
    b_dev, _ = _lay(dev, [b[21]], [BASE_LEN], ROW_STRIDE, 0, CANARY, [pos], other)
    d_len = dev.up(lens)
    maxdiff, sumsq, bad = gpu_ctx.compare(a_dev, b_dev, ROW_STRIDE, d_len, d_len, n_rows)
    want = np.zeros(n_rows, np.float32)
    want[pos] = np.float32(1e-45)
    _same(maxdiff, want, "maxdiff")
    _same(sumsq, want.astype(np.float64) ** 2, "sumsq")
    assert not bad.any() and sumsq[pos] > 0


def test_compare_arguments(gpu_ctx, dev):
    lib = G.load()
    assert lib.grail_batch_compare(gpu_ctx.handle, None, None, 0, None, None, 0, None, None, None) == G.OK
    d_a, d_b = dev.up(np.zeros(128, np.float32)), dev.up(np.ones(128, np.float32))
    d_len = dev.up(np.array([64], np.uint32))
    good = [d_a, d_b, 64, d_len, d_len, 1]
    for k in (0, 1, 3, 4):
        args = list(good)
        args[k] = None
        with pytest.raises(G.GrailError) as ei:
            gpu_ctx.compare(*args)
        assert ei.value.status == G.ERR_INVALID_ARG, k
    maxdiff, sumsq, bad = gpu_ctx.compare(*good)
    assert (maxdiff[0], sumsq[0], bad[0]) == (1.0, 64.0, 0)


# ---- pcm16 -----------------------------------------------------------------------------------------------------------
PCM_LAYOUTS = {                                       # in_stride, out_stride, floats / samples past an aligned base
    "vector path throughout": (10048, 10048, 0, 0),
    "input base + 1 float": (10048, 10048, 1, 0),
    "output base + 1 sample": (10048, 10048, 0, 1),
    "output base + 4 samples": (10048, 10048, 0, 4),  # 8-byte but not 16-byte aligned
    "both strides odd": (10001, 10001, 0, 0),         # the alignment differs row by row
    "strides differ": (10008, 10056, 0, 0),
}


@pytest.fixture(scope="module")
def pcm():
    rows = pcm16_rows()
    return dict(rows=rows, lens=np.array([len(r) for r in rows], np.uint32), want=[pcm16_model(r) for r in rows])


@pytest.mark.parametrize("layout", list(PCM_LAYOUTS))
def test_pcm16_at_every_codes_boundaries(gpu_ctx, dev, pcm, layout):
    """for every k of -32768 ... 32768 the binary32 value nearest k / 32767 and its two neighbours, +-0.0, +-1e-45, +-1.0,
    +-(1 + 2^-23), +-2.0, +-3e38, +-Inf and NaN (about 200 000 samples in rows of 0, 1, 7, 8, 9, 2047, 2048, 2049, 4097 and
    10 000): every output sample equals the model (multiply by 32767.0f, truncate toward zero, clamp, NaN -> 0), every int16
    outside the rows' samples keeps 0x5555 — in front of a shifted base, between the rows, after the last one — whichever
    of the vector and the scalar path the layout's addresses take"""
    in_stride, out_stride, in_off, out_off = PCM_LAYOUTS[layout]
    rows, lens, n = pcm["rows"], pcm["lens"], len(pcm["rows"])
    assert lens.max() <= min(in_stride, out_stride)
    if layout == "vector path throughout":
        assert in_stride % 8 == 0 and out_stride % 8 == 0
    host = np.full(in_off + n * in_stride + 8, 0.75, np.float32)
    total = out_off + n * out_stride + 64
    want = np.full(total, 0x5555, np.int16)
    inside = np.zeros(total, bool)
    for u, x in enumerate(rows):
        host[in_off + u * in_stride:in_off + u * in_stride + len(x)] = x
        want[out_off + u * out_stride:out_off + u * out_stride + len(x)] = pcm["want"][u]
        inside[out_off + u * out_stride:out_off + u * out_stride + len(x)] = True
    d_in, d_out = dev.up(host), dev.alloc(total * 2)
    gpu_ctx.memset(d_out, 0x55, total * 2)
    gpu_ctx.pcm16(C.c_void_p(d_in.value + in_off * 4), in_stride, dev.up(lens), n, int(lens.max()),
                  C.c_void_p(d_out.value + out_off * 2), out_stride)
    gpu_ctx.sync()
    got = dev.down(d_out, total, np.int16)
    for u, x in enumerate(rows):
        g = got[out_off + u * out_stride:out_off + u * out_stride + len(x)]
        miss = np.nonzero(g != pcm["want"][u])[0]
        assert len(miss) == 0, (f"{layout}: row {u} of {len(x)} samples, {len(miss)} differ, first at {miss[0]}: "
                                f"{x[miss[0]]!r} * 32767 = {float(x[miss[0]]) * 32767.0!r} -> {g[miss[0]]}, want {pcm['want'][u][miss[0]]}")
    touched = np.nonzero((got != 0x5555) & ~inside)[0]
    assert len(touched) == 0, f"{layout}: {len(touched)} samples outside the rows were written, first at int16 index {touched[0]}"
    assert np.array_equal(got, want)
