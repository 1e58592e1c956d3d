"""Sample-rate conversion on the device (grail_resample_async) against the numpy model of tests/resample_model.py, bit for
bit in the resampled samples, the lengths and the non-finite counts: rows shorter than the filter, rows that end at, before
and after a seam of the kernel's chunks, impulses, -0.0 and denormals, non-finite samples at the rows' ends and at the
seams; every layout the same bits; nothing written past a row's outputs; an output cut short by out_stride; a row long
enough that m * D passes 2^32; rendered speech through the chain; the table cache."""
import ctypes as C
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import grail_hip as G
from grail_hip import workload as W
from resample_model import resample_model
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)
from test_loudness_host import gate_model, kweight_hops_model, lufs_model
from test_true_peak_host import db, true_peak_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = G.RESAMPLE_CHUNK
# (48000, 2000) and (50, 3) are beside the issue's pairs: their chunks reach further than LDS holds, so the kernel reads the
# row itself, with one phase and with three
PAIRS = [(2, 3), (3, 2), (48000, 16000), (48000, 96000), (44100, 48000), (48000, 44100), (44100, 16000), (48000, 2000), (50, 3)]
LAYOUT_PAIRS = [(48000, 16000), (44100, 48000), (44100, 16000), (50, 3), (48000, 2000)]
LDS_MAX, STAGE_SLACK = 65536 - 64, 8             # resample_kernels.hip's RS_LDS_MAX and RS_STAGE_SLACK (test_kernel_paths_host.py)
VARIANTS = ([("staged", vec, tab) for tab in ("uniform", "lds", "global") for vec in (True, False)] +
            [("unstaged", vec, tab) for tab in ("uniform", "global") for vec in (True, False)])
_tables = {}


def variant(U, D, P, aligned):
    """the resample_kernel<STAGED, VEC, TAB> that launch_resample starts for a ratio U / D with P taps a phase; aligned: both
    bases 16-byte aligned and both strides multiples of 4"""
    stretch = (U - 1 + (CHUNK - 1) * D) // U + P + STAGE_SLACK
    staged_bytes, table_bytes = (CHUNK + stretch) * 4, U * (P + 1) * 4
    staged = staged_bytes <= LDS_MAX
    tab = "uniform" if U == 1 else ("lds" if staged and staged_bytes + table_bytes <= LDS_MAX else "global")
    return ("staged" if staged else "unstaged", bool(aligned), tab)


def table(pair):
    """(numerators int32[U, P], U, D, P), from the library, once per pair"""
    if pair not in _tables:
        U, D, P = G.resample_ratio(*pair)
        _tables[pair] = (G.resample_coefficients(*pair), U, D, P)
    return _tables[pair]


def lengths(pair):
    """the issue's row lengths: Ci = the input samples of one chunk"""
    _, U, D, P = table(pair)
    Ci = -(-CHUNK * D // U)
    return [0, 1, 2, P // 2 - 1, P // 2, P // 2 + 1, Ci - 1, Ci, Ci + 1, 3 * Ci + 17]


def seams(pair, n):
    """the input times either side of every chunk seam inside a row of n samples"""
    _, U, D, _ = table(pair)
    at = set()
    for c in range(1, n * U // D // CHUNK + 2):
        lo, hi = c * CHUNK * D // U, -(-c * CHUNK * D // U)
        at |= {lo - 1, lo, hi, hi + 1}
    return sorted(t for t in at if 0 <= t < n)


def contents(pair, n, rng):
    """the four kinds of row of n samples"""
    noise = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    impulses = np.zeros(n, np.float32)
    small = noise.copy()
    small[rng.random(n) < 0.2] = np.float32(-0.0)
    tiny = rng.random(n) < 0.2
    small[tiny] = (rng.integers(1, 1 << 23, int(tiny.sum())).astype(np.uint32) | (rng.integers(0, 2, int(tiny.sum())).astype(np.uint32) << 31)).view(np.float32)
    holes = noise.copy()
    if n:
        impulses[0] = 1.0
        impulses[n - 1] = -1.0
        for i, t in enumerate([0, n - 1] + seams(pair, n)):
            holes[t] = (np.nan, np.inf, -np.inf)[i % 3]
    return [noise, impulses, small, holes]


def run(ctx, dev, rows, pair, stride=None, out_stride=None, in_offset=0, out_offset=0, guard=64, lens=None):
    """rows[i] as row i of a buffer that holds NaN everywhere else, resampled into a buffer that holds CANARY, with `guard`
    floats of it before and after -> (out [n_rows, out_stride] as it lies on the device afterwards, out_len, nonfinite)"""
    _, U, D, _ = table(pair)
    longest = max([len(x) for x in rows] + [1])
    stride = stride or (longest + 63) // 64 * 64
    out_stride = (-(-longest * U // D) + 63) // 64 * 64 if out_stride is None else out_stride
    host = np.full(len(rows) * stride + in_offset, np.nan, np.float32)
    for i, x in enumerate(rows):
        host[in_offset + i * stride:in_offset + i * stride + len(x)] = x
    d_in = dev.up(host)
    before = guard + out_offset
    d_out = dev.up(np.full(before + len(rows) * out_stride + guard, CANARY, np.float32))
    d_len = dev.up(np.array([len(x) for x in rows] if lens is None else lens, np.uint32))
    out_len, bad = ctx.resample(C.c_void_p(d_in.value + in_offset * 4), stride, d_len, len(rows), pair[0], pair[1],
                                C.c_void_p(d_out.value + before * 4), out_stride)
    out = dev.down(d_out, before + len(rows) * out_stride + guard, np.float32)
    assert np.all(out[:before] == CANARY) and np.all(out[before + len(rows) * out_stride:] == CANARY), "written outside out"
    return out[before:before + len(rows) * out_stride].reshape(len(rows), out_stride), out_len, bad


def same(rows, pair, got, what, out_stride=None):
    """the device's (out, out_len, nonfinite) against the model's; out rows hold the canary past their outputs"""
    num, _, D, _ = table(pair)
    out, out_len, bad = got
    for i, x in enumerate(rows):
        y, n_out, w_bad = resample_model(x, num, D, out_stride=out_stride)
        assert (out_len[i], bad[i]) == (n_out, w_bad), (what, i, len(x), out_len[i], n_out, bad[i], w_bad)
        assert np.all(out[i, n_out:] == CANARY), (what, i, len(x), "written past the row's outputs")
        differ = np.flatnonzero(out[i, :n_out].view(np.uint32) != y.view(np.uint32))
        assert len(differ) == 0, (what, i, len(x), n_out, differ[:8], out[i, differ[:4]], y[differ[:4]])


# ---- 1. bit parity with the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS)
def test_bit_parity_with_the_model(gpu_ctx, dev, pair):
    """one call over rows of the issue's ten lengths in the four kinds of content"""
    rng = np.random.default_rng(pair[0] + pair[1])
    rows = [x for n in lengths(pair) for x in contents(pair, n, rng)]
    num, _, D, _ = table(pair)
    assert sum(resample_model(x, num, D, m_hi=0)[2] for x in rows) > 20
    same(rows, pair, run(gpu_ctx, dev, rows, pair), pair)


# ---- 2. layout independence ---------------------------------------------------------------------------------------------
def test_the_pairs_and_layouts_reach_every_variant_of_the_kernel():
    """launch_resample's arithmetic over what the parity test (every pair, aligned) and the layout test (its pairs: aligned,
    bases one float off, odd strides) pass: all ten variants that can be launched are started by one of them"""
    reached = {variant(*table(pair)[1:], True) for pair in PAIRS}
    reached |= {variant(*table(pair)[1:], aligned) for pair in LAYOUT_PAIRS for aligned in (True, False, False)}
    assert len(VARIANTS) == 10 and reached == set(VARIANTS), sorted(set(VARIANTS) - reached)
    assert variant(*table((48000, 2000))[1:], False) == ("unstaged", False, "uniform")
    assert variant(*table((50, 3))[1:], False) == ("unstaged", False, "global") and table((50, 3))[1] == 3


@pytest.mark.parametrize("pair", LAYOUT_PAIRS)
def test_every_layout_gives_the_same_bits(gpu_ctx, dev, pair):
    """aligned bases and strides that are multiples of 4; bases one float off; odd strides and an out_stride above what the
    rows need"""
    rng = np.random.default_rng(7)
    _, U, D, _ = table(pair)
    ns = lengths(pair)
    rows = [contents(pair, n, rng)[3] for n in (ns[3], ns[7], ns[8], ns[9])]
    need = -(-ns[9] * U // D)
    a = run(gpu_ctx, dev, rows, pair)
    same(rows, pair, a, (pair, "aligned"))
    b = run(gpu_ctx, dev, rows, pair, in_offset=1, out_offset=1)
    c = run(gpu_ctx, dev, rows, pair, stride=ns[9] + 3 - ns[9] % 2, out_stride=need + 131 - need % 2)
    for other, what in ((b, "offset"), (c, "odd strides")):
        same(rows, pair, other, (pair, what))
        assert np.array_equal(other[1], a[1]) and np.array_equal(other[2], a[2])
        for i, n_out in enumerate(a[1]):
            assert np.array_equal(other[0][i, :n_out].view(np.uint32), a[0][i, :n_out].view(np.uint32)), (pair, what, i)


# ---- 3. footprint ---------------------------------------------------------------------------------------------------------
def test_nothing_is_written_outside_the_rows_outputs_and_nothing_read_past_their_samples(gpu_ctx, dev):
    """run() keeps guards of the canary around out and NaN between a row's samples and its stride, same() looks at every
    sample past out_len; here also with len above the stride (the stride bounds the row) and rows of no samples"""
    pair = (48000, 16000)
    rng = np.random.default_rng(11)
    rows = [rng.uniform(-1, 1, n).astype(np.float32) for n in (3072 + 64, 0, 3072 + 64, 5, 3072 + 64)]
    got = run(gpu_ctx, dev, rows, pair, stride=3072 + 64, out_stride=1024 + 64, guard=4096,
              lens=[0xFFFFFFFF, 0, 3072 + 64, 5, 2 ** 31])
    same(rows, pair, got, "len above the stride")
    assert list(got[1]) == [1046, 0, 1046, 2, 1046] and not got[2].any()
    d_len = dev.up(np.zeros(3, np.uint32))
    out_len, bad = gpu_ctx.resample(None, 0, d_len, 3, 48000, 16000, None, 0)        # no samples at all: NULL rows are fine
    assert not out_len.any() and not bad.any()
    gpu_ctx.resample_async(None, 64, None, 0, 48000, 16000, None, 64)                # no rows: nothing queued


# ---- 4. the clamp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(48000, 16000), (44100, 48000), (48000, 2000), (50, 3)])
def test_an_out_stride_below_the_rows_length_gives_the_prefix(gpu_ctx, dev, pair):
    """out_len = out_stride, the samples the prefix of the unclamped result; the non-finite count is that of the whole row,
    also of the samples whose outputs were cut.  (48000, 2000) and (50, 3) are not staged: a cut row's remaining samples are
    counted from the row itself, with one phase and with three"""
    rng = np.random.default_rng(13)
    _, U, D, P = table(pair)
    assert variant(U, D, P, True)[0] == ("unstaged" if pair in ((48000, 2000), (50, 3)) else "staged")
    ns = lengths(pair)
    rows = [contents(pair, ns[9], rng)[3], contents(pair, ns[7], rng)[0], contents(pair, ns[4], rng)[3]]
    rows[0][-5] = np.nan
    full = run(gpu_ctx, dev, rows, pair)
    for out_stride in (CHUNK + 4, CHUNK - 1, 7, 0):
        cut = run(gpu_ctx, dev, rows, pair, out_stride=out_stride)
        same(rows, pair, cut, (pair, out_stride), out_stride=out_stride)
        assert np.array_equal(cut[2], full[2]) and cut[1][0] == out_stride
        for i in range(len(rows)):
            k = cut[1][i]
            assert k == min(full[1][i], out_stride)
            assert np.array_equal(cut[0][i, :k].view(np.uint32), full[0][i, :k].view(np.uint32))


# ---- 5. 64-bit indexing ---------------------------------------------------------------------------------------------------
def test_a_lone_long_row_whose_m_times_d_passes_2_to_the_32(gpu_ctx, dev):
    """44 100 -> 16 000 over 27.2 million samples: a = m * 441 passes 2^32 at m = 9 739 270; 4096 outputs around it and the
    last 4096 against the model, which computes any range of m"""
    pair = (44100, 16000)
    num, U, D, P = table(pair)
    n = 27_200_000
    t = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = (t * np.uint32(2654435761)) ^ (t >> np.uint32(7))
    x = ((h >> np.uint32(8)) & np.uint32(0xFFFF)).astype(np.float32) / np.float32(32768.0) - np.float32(1.0)
    n_out = -(-n * U // D)
    cross = -(-2 ** 32 // D)
    assert (n_out - 1) * D > 2 ** 32 + 4096 * D and cross + 2048 < n_out
    d_in, d_len = dev.up(x), dev.up(np.array([n], np.uint32))
    out_stride = (n_out + 3) // 4 * 4
    d_out = dev.alloc(out_stride * 4)
    out_len, bad = gpu_ctx.resample(d_in, n, d_len, 1, pair[0], pair[1], d_out, out_stride)
    assert (out_len[0], bad[0]) == (n_out, 0)
    for lo in (cross - 2048, n_out - 4096):
        got = dev.down(d_out, 4096, np.float32, offset=lo * 4)
        want, _, _ = resample_model(x, num, D, m_lo=lo, m_hi=lo + 4096)
        differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert len(differ) == 0, (lo, differ[:8], got[differ[:4]], want[differ[:4]])
        assert np.abs(want).max() > 0.1


# ---- 6. the chain -----------------------------------------------------------------------------------------------------------
def test_rendered_speech_resampled_measures_as_the_models_say(gpu_ctx, dev):
    """four rows of the generic voice at 48 kHz, half a second each, resampled to 16 kHz: the model's bits on the rendered
    samples; the true peak and the gated loudness of the result as their models read the resampled rows.  Printed (-s) for
    DESIGN.md §4.13: how far the peak and the loudness moved."""
    rate_in, rate_out, n = 48000, 16000, 4
    num, U, D, _ = table((rate_in, rate_out))
    gpu_ctx.set_voices(W.single_voice(sample_rate=rate_in))
    segs, offs, vids, seeds = W.make_batch(n, sample_rate=rate_in, length=0.125, blend_length=0.125)
    stride = W.max_samples(length=0.125, sample_rate=rate_in)
    out_stride = (-(-stride * U // D) + 63) // 64 * 64
    b = gpu_ctx.upload(segs, offs, vids, seeds)
    try:
        d_rows, d_len = dev.alloc(n * stride * 4), dev.alloc(n * 4)
        d_out = dev.up(np.full(n * out_stride, CANARY, np.float32))
        b.synthesize_async(d_rows, stride, d_len)
        d_out_len = dev.alloc(n * 4)
        gpu_ctx.resample_async(d_rows, stride, d_len, n, rate_in, rate_out, d_out, out_stride, d_out_len, None)
        tp_out, _ = gpu_ctx.true_peak(d_out, out_stride, d_out_len, n)
        gated_out, _, _ = gpu_ctx.loudness(d_out, out_stride, d_out_len, n, rate_out)
        tp_in, _ = gpu_ctx.true_peak(d_rows, stride, d_len, n)
        gated_in, _, _ = gpu_ctx.loudness(d_rows, stride, d_len, n, rate_in)
    finally:
        b.free()
    lens = dev.down(d_len, n, np.uint32)
    rows = dev.down(d_rows, (n, stride), np.float32)
    out = dev.down(d_out, (n, out_stride), np.float32)
    out_len = dev.down(d_out_len, n, np.uint32)
    assert lens.min() > 20000
    coef = G.kweighting(rate_out)
    for i in range(n):
        y, n_out, _ = resample_model(rows[i, :lens[i]], num, D)
        assert out_len[i] == n_out and np.all(out[i, n_out:] == CANARY)
        assert np.array_equal(out[i, :n_out].view(np.uint32), y.view(np.uint32)), i
        assert tp_out[i] == true_peak_model(y)[0]
        hops, _ = kweight_hops_model([y], rate_out, coef)[0]
        assert gated_out[i] == gate_model(hops, rate_out // 10) and gated_out[i] > 0
        print(f"\nrow {i}: {lens[i]} samples at {rate_in} -> {n_out} at {rate_out}: true peak {db(tp_in[i]):+.4f} -> {db(tp_out[i]):+.4f} dBTP "
              f"({db(tp_out[i] / tp_in[i]):+.4f} dB), loudness {lufs_model(gated_in[i]):+.4f} -> {lufs_model(gated_out[i]):+.4f} LUFS "
              f"({lufs_model(gated_out[i]) - lufs_model(gated_in[i]):+.4f} LU)", end="")


# ---- 7. scratch and reuse -------------------------------------------------------------------------------------------------
def test_the_table_cache_is_hit_and_evicted_without_effect(built):
    """a context of its own: a pair, five others (the cache holds four), the first again: the same bits each time; rows that
    need more scratch than the call before; grail_destroy afterwards is clean"""
    rng = np.random.default_rng(17)
    with G.Context(0) as ctx:
        d = Dev(ctx)
        try:
            first = (48000, 16000)
            rows = [contents(first, n, rng)[3] for n in (700, 3072 * 2 + 5)]
            a = run(ctx, d, rows, first)
            same(rows, first, a, "first")
            for pair in [(44100, 48000), (2, 3), (3, 2), (48000, 96000), (48000, 44100), (44100, 48000)]:
                more = [contents(pair, n, rng)[0] for n in (900, 2500)]
                same(more, pair, run(ctx, d, more, pair), pair)
            again = run(ctx, d, rows, first)
            same(rows, first, again, "again")
            assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, again))
            longer = rows + [contents(first, 3072 * 5 + 1, rng)[3] for _ in range(6)]
            same(longer, first, run(ctx, d, longer, first), "more scratch")
        finally:
            d.free()


# ---- the example -----------------------------------------------------------------------------------------------------------
def test_grail_dialogue_rate_option(gpu_ctx, tmp_path):
    """--lufs -23 --ceiling -1 --limit --rate 16000 --report: a 16 kHz WAV of ceil(n * 160 / 441) frames, the line the
    program prints, the report measured at 16 kHz (its true peak is the one the --rate line states); without --rate the
    file is at the voices' 44 100 Hz, and --rate 44100 is the same file"""
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    args = ["--lufs", "-23", "--ceiling", "-1", "--limit", "--report", "hello there", "a fine day to you"]
    runs = {}
    for name, extra in (("plain", []), ("low", ["--rate", "16000"]), ("same", ["--rate", "44100"])):
        r = subprocess.run([exe, "-o", str(tmp_path / f"{name}.wav")] + extra + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        with wave.open(str(tmp_path / f"{name}.wav"), "rb") as w:
            runs[name] = (r.stdout, w.getframerate(), w.getnframes(), w.getnchannels())
    assert runs["plain"][1:] == runs["same"][1:] and runs["plain"][1] == 44100 and runs["plain"][3] == 2
    assert (tmp_path / "plain.wav").read_bytes() == (tmp_path / "same.wav").read_bytes()
    out, rate, frames, channels = runs["low"]
    assert (rate, channels) == (16000, 2) and frames == -(-runs["plain"][2] * 160 // 441)
    m = re.search(r"Resampled from 44100 to 16000 Hz: (\d+) samples a track; track true peaks (\S+) and (\S+) dBTP", out)
    assert m and int(m.group(1)) == frames, out
    assert "Resampled" not in runs["plain"][0] and "Resampled" not in runs["same"][0]
    peaks = re.findall(r"Track \d: .* true peak (\S+) dBTP", out)
    assert len(peaks) == 2 and all(abs(float(p) - float(q)) <= 0.0051 for p, q in zip(peaks, m.group(2, 3))), (m.group(0), peaks)
    print("\n" + m.group(0))
