"""Levels without a GPU (include/grail_hip.h, "levels"): grail_level_gains and grail_active_level against numpy's binary64
formulas, the ctypes signatures, the device entry points failing loudly without a device, and csrc/level_gains.cpp built
with g++ under AddressSanitizer + UBSan and driven by tests/sanitize_levels_driver.cpp.

Also the numpy model of the contract, written from the header's words, that tests/test_levels_gpu.py compares the device
with: frame_model() and row_model()."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grail_hip as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.float32(3.4028234663852886e38)


# ---- the contract in numpy -------------------------------------------------------------------------------------------
def frame_model(x, frame):
    """(sumsq float64[frames], peak float32[frames], nonfinite[frames]) of one row x (float32) for frames of `frame`
    samples.  Per frame: 256 partials p[t mod 256], t counted from the row's first sample, each the left fold in ascending
    t of p + (double)x * (double)x over the finite samples; then the halving tree w = 128 ... 1.  The frame is laid out
    as rows of 256 (zeros before its first and after its last sample, and in place of non-finite samples: a partial is
    never negative, so adding +0.0 is the same as skipping) and the rows are added one after the other — never np.sum,
    which adds pairwise."""
    x = np.asarray(x, np.float32)
    n = len(x)
    frames = -(-n // frame)
    sumsq, peak, bad = np.zeros(frames, np.float64), np.zeros(frames, np.float32), np.zeros(frames, np.uint32)
    for f in range(frames):
        start, end = f * frame, min((f + 1) * frame, n)
        seg = x[start:end]
        with np.errstate(invalid="ignore"):
            finite = np.abs(seg) <= FLT_MAX
        v = np.where(finite, seg, np.float32(0.0)).astype(np.float64)
        front = start % 256
        buf = np.zeros(-(-(front + len(seg)) // 256) * 256, np.float64)
        buf[front:front + len(seg)] = v * v                      # (exact: 24-bit significands)
        p = np.zeros(256, np.float64)
        for chunk in buf.reshape(-1, 256):
            p = p + chunk
        w = 128
        while w >= 1:
            p[:w] = p[:w] + p[w:2 * w]
            w //= 2
        sumsq[f] = p[0]
        peak[f] = np.abs(seg[finite]).max() if finite.any() else np.float32(0.0)
        bad[f] = np.count_nonzero(~finite)
    return sumsq, peak, bad


def row_model(x):
    """(sumsq, peak, nonfinite) of one row: the frames of GRAIL_LEVEL_FRAME samples, their sums folded in ascending order"""
    fs, fp, fb = frame_model(x, G.LEVEL_FRAME)
    s = np.float64(0.0)
    for v in fs:
        s = s + v
    return s, (fp.max() if len(fp) else np.float32(0.0)), int(fb.sum())


def gains_model(mode, level_db, rows, sumsq=None, peak=None, nonfinite=None, row_len=None, active=None):
    """the header's formula in binary64, rounded once to binary32; (gains, n_unleveled)"""
    rows = np.asarray(rows)
    if mode == G.LEVEL_PEAK:
        level = np.asarray(peak, np.float64)
    elif mode == G.LEVEL_RMS:
        ln = np.asarray(row_len, np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            level = np.where(ln > 0, np.sqrt(np.asarray(sumsq, np.float64) / ln), 0.0)
    else:
        level = np.asarray(active, np.float64)
    out = ~(level > 0)
    if nonfinite is not None:
        out |= np.asarray(nonfinite) != 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        g = (10.0 ** (np.asarray(level_db, np.float32).astype(np.float64) / 20.0) / level[rows]).astype(np.float32)
    g[out[rows]] = 0.0
    return g, int(out[rows].sum())


def within_one_ulp(a, b):
    """binary32 values at most one unit in the last place apart (the C library's pow and numpy's may differ in the last
    bit of binary64, which can move the rounding to binary32 by one)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return a.shape == b.shape and bool(np.all(np.abs(ia - ib) <= 1))


# ---- the model itself -------------------------------------------------------------------------------------------------
def test_model_is_a_sum_of_squares_and_ignores_what_the_contract_says_it_ignores():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(10007).astype(np.float32)
    s, p, b = row_model(x)
    assert abs(s - float(np.sum(x.astype(np.float64) ** 2))) <= 1e-12 * s and p == np.abs(x).max() and b == 0
    y = x.copy()
    y[[5, 4096, 10006]] = [np.nan, np.inf, -np.inf]
    z = x.copy()
    z[[5, 4096, 10006]] = [0.0, -0.0, 0.0]
    sy, py, by = row_model(y)
    sz, pz, bz = row_model(z)
    assert by == 3 and bz == 0 and sy == sz and py == pz                     # skipped = +0.0 in its place
    for frame in (256, 441, 4096):
        fs, fp, fb = frame_model(x, frame)
        assert len(fs) == -(-len(x) // frame)
        assert abs(fs.sum() - s) <= 1e-12 * s and fp.max() == p
    assert row_model(np.zeros(0, np.float32)) == (0.0, 0.0, 0)


# ---- grail_level_gains ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_level_gains_equal_the_binary64_formula(built, seed):
    rng = np.random.default_rng(seed)
    n_rows, n_items = int(rng.integers(1, 60)), int(rng.integers(1, 400))
    row_len = rng.integers(1, 200000, n_rows).astype(np.uint32)
    peak = (rng.uniform(0.01, 2.0, n_rows) * np.exp2(rng.integers(-20, 4, n_rows))).astype(np.float32)
    sumsq = rng.uniform(1e-6, 0.5, n_rows) * row_len
    bad = np.zeros(n_rows, np.uint32)
    rows = rng.integers(0, n_rows, n_items).astype(np.uint32)
    db = rng.uniform(-60, 12, n_items).astype(np.float32)
    for mode, kw in ((G.LEVEL_PEAK, dict(peak=peak)), (G.LEVEL_RMS, dict(sumsq=sumsq, row_len=row_len))):
        got, out = G.level_gains(mode, rows, db, nonfinite=bad, **kw)
        want, want_out = gains_model(mode, db, rows, nonfinite=bad, **kw)
        assert out == want_out == 0
        assert within_one_ulp(got, want), np.max(np.abs(got - want))
        assert np.all(got > 0)
    # the arrays a mode does not need may be NULL; so may nonfinite
    got2, _ = G.level_gains(G.LEVEL_PEAK, rows, db, peak=peak)
    assert np.array_equal(got2, G.level_gains(G.LEVEL_PEAK, rows, db, peak=peak, nonfinite=bad, sumsq=sumsq, row_len=row_len)[0])


def test_rows_that_cannot_be_leveled_get_gain_zero_and_are_counted(built):
    # row 0: silent; row 1: empty; row 2: holds a non-finite sample; row 3: fine
    sumsq = np.array([0.0, 0.0, 4.0, 4.0])
    peak = np.array([0.0, 0.0, 1.0, 1.0], np.float32)
    bad = np.array([0, 0, 2, 0], np.uint32)
    row_len = np.array([100, 0, 100, 100], np.uint32)
    active = np.array([0.0, 0.0, 0.2, 0.2])
    rows = np.array([3, 0, 1, 2, 2, 3, 0], np.uint32)
    db = np.full(len(rows), -20.0, np.float32)
    for mode in (G.LEVEL_PEAK, G.LEVEL_RMS, G.LEVEL_ACTIVE):
        g, out = G.level_gains(mode, rows, db, sumsq=sumsq, peak=peak, nonfinite=bad, row_len=row_len, active_level=active)
        assert out == 5                                                          # items, not rows
        assert np.array_equal(g[[1, 2, 3, 4, 6]], np.zeros(5, np.float32)) and g[0] == g[5] > 0
        level = {G.LEVEL_PEAK: 1.0, G.LEVEL_RMS: 0.2, G.LEVEL_ACTIVE: 0.2}[mode]
        assert within_one_ulp(g[0], np.float32(10.0 ** (-20.0 / 20.0) / level))
    # a row of one empty sample count but a sum (inconsistent input) must not divide by zero
    g, out = G.level_gains(G.LEVEL_RMS, [1], [0.0], sumsq=[1.0, 1.0], row_len=[5, 0])
    assert g[0] == 0 and out == 1


def test_invalid_arguments_leave_the_gains_unwritten(built):
    lib = G.load()
    peak = np.ones(3, np.float32)
    sumsq, row_len = np.ones(3), np.full(3, 10, np.uint32)
    db = np.zeros(4, np.float32)
    for rows in ([0, 1, 2, 3], [0xFFFFFFFF, 0, 0, 0]):                       # an item row past n_rows
        rows = np.array(rows, np.uint32)
        g = np.full(4, -5.0, np.float32)
        out = C.c_uint32(99)
        rc = lib.grail_level_gains(G.LEVEL_PEAK, None, peak.ctypes.data, None, None, None, 3, rows.ctypes.data,
                                   db.ctypes.data, 4, g.ctypes.data, C.addressof(out))
        assert rc == G.ERR_INVALID_ARG and np.all(g == -5.0) and out.value == 99
        with pytest.raises(G.GrailError) as ei:
            G.level_gains(G.LEVEL_RMS, rows, db, sumsq=sumsq, row_len=row_len)
        assert ei.value.status == G.ERR_INVALID_ARG
    rows = np.zeros(4, np.uint32)
    g = np.full(4, -5.0, np.float32)
    for mode, args in ((7, (sumsq.ctypes.data, peak.ctypes.data, None, row_len.ctypes.data, None)),      # unknown mode
                       (G.LEVEL_PEAK, (sumsq.ctypes.data, None, None, row_len.ctypes.data, None)),      # no peak
                       (G.LEVEL_RMS, (sumsq.ctypes.data, peak.ctypes.data, None, None, None)),          # no row_len
                       (G.LEVEL_ACTIVE, (sumsq.ctypes.data, peak.ctypes.data, None, row_len.ctypes.data, None))):
        assert lib.grail_level_gains(mode, *args, 3, rows.ctypes.data, db.ctypes.data, 4, g.ctypes.data, None) == G.ERR_INVALID_ARG
        assert np.all(g == -5.0)
    assert lib.grail_level_gains(G.LEVEL_PEAK, None, None, None, None, None, 0, None, None, 0, None, None) == G.OK


# ---- grail_active_level -----------------------------------------------------------------------------------------------
def test_active_level_of_a_row_that_is_half_silence(built):
    """16 frames of 4096 with a mean square of 0.04 and 16 silent ones: the whole-row RMS halves the mean square, the
    active level does not: 10 log10(2) = 3.01 dB above"""
    frame = 4096
    fs = np.concatenate([np.full(16, 0.04 * frame), np.zeros(16)])
    rng = np.random.default_rng(2)
    fs = fs[rng.permutation(32)]
    n = 32 * frame
    act = G.active_level(fs, n, frame, 40.0)
    rms = np.sqrt(fs.sum() / n)
    assert abs(act - 0.2) < 1e-15
    assert abs(20 * np.log10(act / rms) - 3.0103) < 1e-4
    # frames below the floor are left out, frames above it are kept: -39 dB and -41 dB of the loudest
    fs = np.array([1.0, 10 ** -3.9, 10 ** -4.1]) * frame
    want = np.sqrt((fs[0] + fs[1]) / (2 * frame))
    assert G.active_level(fs, 3 * frame, frame, 40.0) == want
    assert G.active_level(fs, 3 * frame, frame, 45.0) == np.sqrt((fs[0] + fs[1] + fs[2]) / (3 * frame))
    assert G.active_level(fs, 3 * frame, frame, 0.0) == 1.0


def test_active_level_weighs_the_short_last_frame_by_its_own_count(built):
    frame, n = 1000, 2100                                   # frames of 1000, 1000 and 100 samples
    # the last frame is the loudest PER SAMPLE although its sum is the smallest
    fs = np.array([1000 * 0.01, 1000 * 1e-7, 100 * 0.04])
    act = G.active_level(fs, n, frame, 40.0)
    s = np.float64(0.0) + fs[0] + fs[2]                     # frame 1: 1e-7 / 0.04 is below -40 dB
    assert act == np.sqrt(s / (1000.0 + 100.0))
    # ... and had it been weighed as a full frame it would have counted as quiet: 0.004 / 0.01, still active; so make it
    # the only loud one
    fs = np.array([1000 * 1e-6, 1000 * 1e-6, 100 * 0.04])
    assert G.active_level(fs, n, frame, 30.0) == np.sqrt(fs[2] / 100.0) == 0.2
    # one sample in the last frame
    assert G.active_level([0.0, 0.25], 1001, 1000, 40.0) == 0.5


def test_active_level_of_silence_and_of_nothing_is_zero(built):
    assert G.active_level(np.zeros(24), 96006, 4096, 40.0) == 0.0
    assert G.active_level(np.zeros(1), 0, 4096, 40.0) == 0.0
    assert G.active_level(np.zeros(0), 0, 4096, 40.0) == 0.0


# ---- the device entry points without a device ---------------------------------------------------------------------------
def test_signatures_load_and_device_calls_fail_loudly_without_a_device(built):
    lib = G.load()
    for name in ("grail_levels_async", "grail_frame_levels_async", "grail_level_gains", "grail_active_level",
                 "grail_batch_mix_leveled"):
        assert name in G.EXPORTS and getattr(lib, name).argtypes is not None
    assert lib.grail_active_level.restype is C.c_double
    assert len(lib.grail_levels_async.argtypes) == 8 and len(lib.grail_frame_levels_async.argtypes) == 9
    assert len(lib.grail_level_gains.argtypes) == 12 and len(lib.grail_batch_mix_leveled.argtypes) == 16
    assert (G.LEVEL_PEAK, G.LEVEL_RMS, G.LEVEL_ACTIVE, G.LEVEL_FRAME) == (0, 1, 2, 4096)
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    for text in ("#define GRAIL_LEVEL_FRAME      4096u", "#define GRAIL_LEVEL_PEAK       0", "#define GRAIL_LEVEL_RMS        1",
                 "#define GRAIL_LEVEL_ACTIVE     2"):
        assert text in hdr
    if G.device_count() == 0:        # no context can exist: the calls say why, they do not compute on the CPU
        assert lib.grail_levels_async(None, None, 64, None, 1, None, None, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_frame_levels_async(None, None, 64, None, 1, 256, None, None, 1) == G.ERR_NO_DEVICE
        assert lib.grail_batch_mix_leveled(None, None, None, None, None, None, G.LEVEL_RMS, 0, None, 0, 0, 0, None, None,
                                           None, 0) == G.ERR_NO_DEVICE
        with pytest.raises(G.GrailError) as ei:
            G.Context(0)
        assert ei.value.status == G.ERR_NO_DEVICE


def test_dialogue_example_knows_the_level_option(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--level DB" in r.stderr
    r = subprocess.run([exe, "--level", "loud", "a", "e"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--level", "-20", "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr


# ---- the host helpers under the sanitizers ------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_level_helpers_under_asan_ubsan(tmp_path):
    """csrc/level_gains.cpp makes no HIP call: built with g++ and the sanitizers, then driven by
    tests/sanitize_levels_driver.cpp over arrays of exactly the documented sizes."""
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-ffp-contract=off", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "level_gains.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_levels_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_levels_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize levels driver: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
