"""grail_spectrum_async on the device against the page of numpy (tests/spectrum_model.py): power, bands, n_frames and nonfinite
bit for bit.  67 rows a set whose lengths sit on every edge (0, 1, W - 1, W, W + 1, H, H + 1, a multiple of H, the stride
itself), the memory behind each length NaN; rows with +-inf, NaN, -0.0, denormals and FLT_MAX in them; an aligned base with a
stride that is a multiple of 4 and a base shifted by one word with an odd stride; power only, bands only and both; one lone
row of 300 000 samples.

Which case reaches which instantiation of spectrum_kernel<P, VEC> (the launcher picks P = the set's log2n, VEC = the rows
start on 16 bytes and lie a multiple of 4 samples apart):
    test_rows_equal_the_model[p6-*]    <6, *>   four frames side by side, a wave each; 19 frames a row: three chunks
    test_rows_equal_the_model[p7-*]    <7, *>   the same, P odd (stage 1 alone), W < N, a lead, hand-made bands
    test_rows_equal_the_model[p10-*]   <10, *>  a frame a workgroup, 80 mel bands, 11 frames a row: two chunks
    test_rows_equal_the_model[p12-*]   <12, *>  96 KB of LDS, W = 4001, an empty band and the single bin N/2
    test_other_sizes_equal_the_model   <8, *>, <9, *>, <11, *>
    test_a_lone_long_row               <10, 1>  147 chunks of one row
([*-vec] is VEC = 1, [*-scalar] VEC = 0.)  spectrum_totals_kernel runs in every call that asks for a result."""
import ctypes as C
import functools

import numpy as np
import pytest

import grail_hip as G
import spectrum_model as M
from grail_hip import spectrum as S
from test_levels_gpu import Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
CANARY_BITS = 0xC0DEFACE                         # (a float32 of about -7: no power is negative, and no band of these sets lands on it)
N_ROWS = 67
FLT_MAX = np.float32(3.4028234663852886e38)


def awkward(rng, n):
    """audio-sized samples with -0.0, denormals, FLT_MAX, NaN and +-Inf sprinkled in (about one sample in forty)"""
    x = (rng.standard_normal(n) * 0.2).astype(np.float32)
    special = np.array([-0.0, 1e-42, -3e-45, FLT_MAX, -FLT_MAX, np.nan, np.inf, -np.inf, 1.0, -1.0], np.float32)
    at = rng.random(n) < 0.025
    x[at] = special[rng.integers(0, len(special), int(at.sum()))]
    return x


def hand_bands(rng, half, n_bands):
    """bands nobody designed: any range inside 0 .. half, weights of either sign, some of them 0 and denormal"""
    first = rng.integers(0, half + 1, n_bands).astype(np.uint32)
    count = np.array([rng.integers(0, half + 2 - f) for f in first], np.uint32)
    weights = (rng.standard_normal(int(count.sum())) * 3).astype(np.float32)
    weights[::7] = 0.0
    weights[3::11] = 1e-40
    return first, count, weights


@functools.lru_cache(maxsize=None)
def the_set(name):
    """(p, window, hop, pad, bands or None, row stride of the aligned layout)"""
    rng = np.random.default_rng(len(name))
    if name == "p6":
        return 6, M.window(M.HANN, 64), 16, 0, None, 300
    if name == "p7":
        return 7, (rng.standard_normal(100) * 2).astype(np.float32), 37, 50, hand_bands(rng, 64, 13), 400
    if name == "p10":
        return 10, M.window(M.HAMMING, 1024), 256, 512, M.mel_design(22050, 10, 80, 0.0, 11025.0), 2600
    if name == "p12":
        half = 2048
        first, count = np.array([7, 100, half], np.uint32), np.array([1500, 0, 1], np.uint32)
        return 12, M.window(M.HANN, 4001), 1000, 0, (first, count, (rng.standard_normal(1501) * 0.5).astype(np.float32)), 9004
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def the_rows(name):
    """the set's 67 rows and what the model makes of them, computed once"""
    p, w, hop, pad, bands, stride = the_set(name)
    W = len(w)
    rng = np.random.default_rng(1000 + p)
    edges = [0, 1, W - 1, W, W + 1, hop, hop + 1, 3 * hop, stride, stride + 1, 8 * hop, 8 * hop + 1, 2]
    lengths = [min(n, stride + 1) for n in edges] + [int(v) for v in rng.integers(0, stride + 2, N_ROWS - len(edges))]
    # (stride + 1 is the odd layout's stride; the aligned layout cuts those rows at its own)
    rows = [awkward(rng, n) for n in lengths]
    rows[20] = np.zeros(stride // 2, np.float32)                        # silence: every bin +0.0
    rows[21] = np.full(stride // 2 + 1, FLT_MAX, np.float32)            # the largest a row can be: power overflows binary32
    return rows, {}


def expected(name, stride):
    rows, cache = the_rows(name)
    if stride not in cache:
        p, w, hop, pad, bands, _ = the_set(name)
        cache[stride] = M.spectrum_model([x[:stride] for x in rows], p, w, hop, pad, *(bands or ()))
    return cache[stride]


def place(dev, rows, stride, offset):
    """the rows at `stride` from a base shifted by `offset` words, NaN wherever no sample lies -> (rows_dev, len_dev)"""
    host = np.full(len(rows) * stride + offset, np.nan, np.float32)
    for i, x in enumerate(rows):
        n = min(len(x), stride)
        host[offset + i * stride:offset + i * stride + n] = x[:n]
    d_len = dev.up(np.array([len(x) for x in rows], np.uint32))         # (a len above the stride is cut at the stride)
    return C.c_void_p(dev.up(host).value + 4 * offset), d_len


def run(ctx, dev, spectrum_set, rows_dev, stride, d_len, n_rows, frames_stride, bins, n_bands, want_power, want_bands):
    """one call -> (power words [n_rows][frames_stride][bins] or None, bands words or None, n_frames, nonfinite)"""
    d_p = dev.up(np.full(n_rows * frames_stride * bins, CANARY_BITS, np.uint32)) if want_power else None
    d_b = dev.up(np.full(n_rows * frames_stride * n_bands, CANARY_BITS, np.uint32)) if want_bands else None
    n_frames, bad = S.transform(ctx, spectrum_set, rows_dev, stride, d_len, n_rows, d_p, d_b, frames_stride)
    power = dev.down(d_p, (n_rows, frames_stride, bins), np.uint32) if want_power else None
    bands = dev.down(d_b, (n_rows, frames_stride, n_bands), np.uint32) if want_bands else None
    return power, bands, n_frames, bad


def check(want, power, bands, n_frames, bad, what):
    for i, (w_power, w_bands, w_frames, w_bad) in enumerate(want):
        assert (n_frames[i], bad[i]) == (w_frames, w_bad), (what, i)
        for got, model in ((power, w_power), (bands, w_bands)):
            if got is None:
                continue
            assert np.array_equal(got[i, :w_frames], model.view(np.uint32)), (what, i, w_frames)
            assert np.all(got[i, w_frames:] == CANARY_BITS), (what, i, "a frame past the row's last was written")


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("name", ["p6", "p7", "p10", "p12"])
def test_rows_equal_the_model(gpu_ctx, dev, name, layout):
    p, w, hop, pad, bands, stride = the_set(name)
    offset = 0
    if layout == "scalar":
        stride, offset = stride + 1, 1
    assert (stride % 4 == 0) == (layout == "vec")
    rows, _ = the_rows(name)
    want = expected(name, stride)
    assert sum(bad for _, _, _, bad in want) > 50 and any(np.isinf(pw).any() for pw, _, _, _ in want)
    bins, n_bands = (1 << p) // 2 + 1, 0 if bands is None else len(bands[0])
    frames_stride = M.frames(stride, hop) + 1
    rows_dev, d_len = place(dev, rows, stride, offset)
    assert (rows_dev.value % 16 == 0) == (layout == "vec")
    spectrum_set = S.create(gpu_ctx, p, w, hop, pad, bands)
    try:
        outputs = [(True, False)] + ([(False, True), (True, True)] if n_bands else [])
        for want_power, want_bands in outputs:
            got = run(gpu_ctx, dev, spectrum_set, rows_dev, stride, d_len, N_ROWS, frames_stride, bins, n_bands, want_power, want_bands)
            check(want, *got, (name, layout, want_power, want_bands))
        # the results are optional too, and without them the outputs are the same
        d_p = dev.up(np.full(N_ROWS * frames_stride * bins, CANARY_BITS, np.uint32))
        S.transform_async(gpu_ctx, spectrum_set, rows_dev, stride, d_len, N_ROWS, d_p, None, frames_stride)
        gpu_ctx.sync()
        check(want, dev.down(d_p, (N_ROWS, frames_stride, bins), np.uint32), None, [t[2] for t in want], [t[3] for t in want], (name, "bare"))
    finally:
        S.free(gpu_ctx, spectrum_set)


@pytest.mark.parametrize("p", [8, 9, 11])
def test_other_sizes_equal_the_model(gpu_ctx, dev, p):
    N = 1 << p
    rng = np.random.default_rng(p)
    w, hop, pad = M.window(M.HANN, N - 3), N // 4 + 1, N // 2
    bands = hand_bands(rng, N // 2, 5)
    for stride, offset in ((3 * N, 0), (3 * N + 1, 1)):
        rows = [awkward(rng, n) for n in (stride, 0, N, stride - 1, 1, 9 * hop + 1)]
        want = M.spectrum_model([x[:stride] for x in rows], p, w, hop, pad, *bands)
        rows_dev, d_len = place(dev, rows, stride, offset)
        frames_stride = M.frames(stride, hop)
        spectrum_set = S.create(gpu_ctx, p, w, hop, pad, bands)
        try:
            got = run(gpu_ctx, dev, spectrum_set, rows_dev, stride, d_len, len(rows), frames_stride, N // 2 + 1, 5, True, True)
        finally:
            S.free(gpu_ctx, spectrum_set)
        check(want, *got, (p, stride))


def test_a_lone_long_row(gpu_ctx, dev):
    p, w, hop, pad, bands, _ = the_set("p10")
    n = 300000
    rng = np.random.default_rng(300000)
    x = awkward(rng, n)
    want = M.spectrum_model([x], p, w, hop, pad, *bands)
    assert want[0][2] == 1172                                            # 147 chunks of 8 frames, the last of 4
    rows_dev, d_len = place(dev, [x], n, 0)
    spectrum_set = S.create(gpu_ctx, p, w, hop, pad, bands)
    try:
        got = run(gpu_ctx, dev, spectrum_set, rows_dev, n, d_len, 1, 1172, 513, 80, True, True)
    finally:
        S.free(gpu_ctx, spectrum_set)
    check(want, *got, "lone")


def test_refusals_that_read_the_set(gpu_ctx, dev):
    """what tests/test_spectrum_host.py cannot reach without a context: the checks that read the set's facts, and the lookup"""
    lib = G.load()
    w = M.window(M.HANN, 64)
    with_bands = S.create(gpu_ctx, 6, w, 16, 0, (np.array([0], np.uint32), np.array([3], np.uint32), np.ones(3, np.float32)))
    bare = S.create(gpu_ctx, 6, w, 16, 0)
    d_rows = dev.up(np.zeros(2 * 64 + 2 * 4 * 33, np.float32))
    d_len, d_out = dev.up(np.array([64, 64], np.uint32)), dev.up(np.full(2 * 4 * 33, CANARY_BITS, np.uint32))
    inside = C.c_void_p(d_rows.value + 4 * 127)
    try:
        for args, word in [((bare, d_rows, 64, d_len, 2, d_out, d_out, 4), b"set of no bands"),
                           ((bare, d_rows, 64, d_len, 2, d_out, None, 3), b"frames_stride"),
                           ((bare, d_rows, 65, d_len, 1, d_out, None, 4), b"frames_stride"),
                           ((bare, d_rows, 64, d_len, 2, None, None, 4), b"both NULL"),
                           ((bare, d_rows, 64, d_len, 2, inside, None, 4), b"power_dev overlaps"),
                           ((with_bands, d_rows, 64, d_len, 2, None, inside, 4), b"bands_dev overlaps"),
                           ((C.c_void_p(bare.value + 8), d_rows, 64, d_len, 2, d_out, None, 4), b"not a spectrum set")]:
            with pytest.raises(G.GrailError) as ei:
                S.transform_async(gpu_ctx, *args)
            assert ei.value.status == G.ERR_INVALID_ARG and word in lib.grail_last_error(), (word, lib.grail_last_error())
        S.transform_async(gpu_ctx, bare, d_rows, 64, d_len, 0, d_out, None, 4)                      # no rows: nothing queued
        gpu_ctx.sync()
        assert np.all(dev.down(d_out, 2 * 4 * 33, np.uint32) == CANARY_BITS)
        with G.Context(0) as other:
            with pytest.raises(G.GrailError) as ei:
                S.transform_async(other, bare, d_rows, 64, d_len, 2, d_out, None, 4)
            assert ei.value.status == G.ERR_INVALID_ARG and b"not a spectrum set" in lib.grail_last_error()
            with pytest.raises(G.GrailError):
                S.free(other, bare)
    finally:
        S.free(gpu_ctx, with_bands)
        S.free(gpu_ctx, bare)
    for stale in (bare, with_bands):                                                           # freed before: looked up, not looked into
        with pytest.raises(G.GrailError) as ei:
            S.free(gpu_ctx, stale)
        assert ei.value.status == G.ERR_INVALID_ARG
        with pytest.raises(G.GrailError) as ei:
            S.transform_async(gpu_ctx, stale, d_rows, 64, d_len, 2, d_out, None, 4)
        assert ei.value.status == G.ERR_INVALID_ARG
    S.free(gpu_ctx, None)
