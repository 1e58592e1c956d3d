"""True peak (include/grail_hip.h, "levels, continued: true peak") without a GPU: the numpy model of the contract that
tests/test_true_peak_gpu.py holds the device to, the table, exact known answers, tones against the tolerance of EBU Tech
3341, the tap-sum bound, grail_true_peak_limit_gains against its model, grail_true_peak_db, the signatures, the example's
usage, and the host functions under AddressSanitizer and UBSan (tests/sanitize_true_peak_driver.cpp)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import grail_hip as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.float32(3.4028234663852886e38)
N0 = [14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68]
N1 = [-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155]
NUMERATORS = np.array([N0, N1, N1[::-1], N0[::-1]], np.int64)       # the header's table, typed again
TAPS = NUMERATORS.astype(np.float64) / 8192.0
TAP_SUM = 16571.0 / 8192.0                                          # the largest sum of |taps| of a phase (phases 1 and 2)
# |y| <= TAP_SUM x max |x| holds for the exact sum; the contract's eleven rounded adds (the first lands on +0.0) can each
# add a relative 2^-53, and the right-hand side below is two rounded products itself: 13 in all, asserted with 16
ROUNDING = 1.0 + 16 * 2.0 ** -53
CANARY = -7.25


def true_peak_model(x):
    """the header's words in numpy's binary64, vectorised over t: per phase acc = acc + C[p][k] * v[t - k] for ascending k
    from +0.0 (element by element the contract's left fold: every product is exact, every add rounded by itself).
    -> (true peak, count of non-finite samples)"""
    x = np.asarray(x, np.float32)
    n = len(x)
    if n == 0:
        return 0.0, 0
    with np.errstate(invalid="ignore"):
        finite = np.abs(x) <= FLT_MAX                               # false for NaN and Inf
    v = np.where(finite, x, np.float32(0.0)).astype(np.float64)
    padded = np.concatenate([np.zeros(11), v, np.zeros(11)])        # v[t] = padded[t + 11]; outputs t = 0 .. n + 10
    best = 0.0
    for p in range(4):
        acc = np.zeros(n + 11)
        for k in range(12):
            acc = acc + TAPS[p, k] * padded[11 - k:11 - k + n + 11]
        best = max(best, float(np.abs(acc).max()))
    return best, int(n - np.count_nonzero(finite))


def ceiling_of(ceiling_db):
    """c of the header: the C library's pow, as the library calls it"""
    return math.pow(10.0, float(np.float32(ceiling_db)) / 20.0)


def limit_model(true_peak, item_rows, gains, ceiling_db):
    """grail_true_peak_limit_gains in numpy: (gains, n_limited)"""
    c = ceiling_of(ceiling_db)
    g = np.array(gains, np.float32)
    limited = 0
    for i, r in enumerate(np.asarray(item_rows)):
        t = float(true_peak[r])
        if not t > 0 or not float(np.abs(g[i])) * t > c:
            continue
        q = np.float32(c / t)
        if float(q) * t > c:
            q = np.nextafter(q, np.float32(0.0))
        g[i] = -q if np.signbit(g[i]) else q
        limited += 1
    return g, limited


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    u = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def db(x):
    return 20.0 * math.log10(x)


def tone(hz, phase_deg, amplitude, rate=48000, seconds=0.5, fade=2000):
    t = np.arange(int(rate * seconds))
    x = amplitude * np.sin(2.0 * np.pi * hz * t / rate + np.deg2rad(phase_deg))
    ramp = np.minimum(1.0, np.minimum(t, t[-1] - t) / float(fade))
    return (x * ramp).astype(np.float32)


# ---- the table --------------------------------------------------------------------------------------------------------------
def test_coefficients_equal_the_table_and_mirror(built):
    coef = G.true_peak_coefficients()
    assert coef.shape == (4, 12) and coef.dtype == np.float64
    assert same_bits(coef, TAPS)
    assert np.array_equal(coef * 8192.0, NUMERATORS)                # integers over 2^13: exact
    assert same_bits(coef[2], coef[1][::-1].copy()) and same_bits(coef[3], coef[0][::-1].copy())
    assert np.abs(NUMERATORS).sum(axis=1).max() == 16571
    assert G.load().grail_true_peak_coefficients(None) == G.ERR_INVALID_ARG
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "#define GRAIL_TRUE_PEAK_PHASES 4" in hdr and "#define GRAIL_TRUE_PEAK_TAPS   12" in hdr
    assert (G.TRUE_PEAK_PHASES, G.TRUE_PEAK_TAPS) == (4, 12)


# ---- exact known answers ----------------------------------------------------------------------------------------------------
def test_exact_known_answers_of_the_model():
    assert true_peak_model(np.zeros(0, np.float32)) == (0.0, 0)
    assert true_peak_model([1.0]) == (7964.0 / 8192.0, 0)
    assert true_peak_model([0.0] * 4095 + [1.0]) == (7964.0 / 8192.0, 0)        # the tail counts (239 / 8192 without it)
    for n in (12, 13, 100, 4096):
        assert true_peak_model(np.ones(n, np.float32)) == (9141.0 / 8192.0, 0), n  # the step overshoot
    assert true_peak_model([-1.0]) == (7964.0 / 8192.0, 0)
    assert true_peak_model([np.nan, np.inf, -np.inf]) == (0.0, 3)
    assert true_peak_model([np.nan, 1.0, np.inf]) == (7964.0 / 8192.0, 2)
    tp, bad = true_peak_model([FLT_MAX] * 12)
    assert bad == 0 and tp == float(FLT_MAX) * 9141.0 / 8192.0 and np.isfinite(tp)
    tp, _ = true_peak_model([np.float32(1e-45)])
    assert tp == float(np.float32(1e-45)) * 7964.0 / 8192.0 and tp > 0      # a binary32 denormal is a sample like any other
    assert true_peak_model([-0.0, 0.0]) == (0.0, 0)


@pytest.mark.parametrize("hz, phase, amplitude, want_db, sample_peak_db",
                         [(12000.0, 45.0, 0.5, -5.976, -9.03), (6000.0, 22.5, 0.5, -6.028, None),
                          (8000.0, 30.0, 0.5, -6.069, None), (997.0, 0.0, 1.0, 0.009, None)])
def test_tones_read_their_amplitude(hz, phase, amplitude, want_db, sample_peak_db):
    """0.5 s at 48 kHz with 2 000-sample linear fades: within +0.2 / -0.4 dB of the amplitude (EBU Tech 3341), and the
    values the issue states to a thousandth of a dB"""
    x = tone(hz, phase, amplitude)
    tp, bad = true_peak_model(x)
    got = db(tp)
    print(f"\n{hz:.0f} Hz at {phase} degrees, amplitude {amplitude}: {got:.4f} dBTP, sample peak {db(np.abs(x).max()):.3f} dB")
    assert bad == 0
    assert -0.4 <= got - db(amplitude) <= 0.2, got
    assert abs(got - want_db) <= 1.5e-3, got
    if sample_peak_db is not None:
        assert abs(db(float(np.abs(x).max())) - sample_peak_db) <= 5e-3


def test_the_tap_sum_bounds_the_true_peak_of_noise():
    """|y| <= sum |C[p][k]| * max |x| (derivable, not measured), times ROUNDING for the binary64 adds"""
    rng = np.random.default_rng(5)
    for n, scale in ((1, 1.0), (13, 0.3), (4096, 1e-3), (100003, 5.0), (5000, 1e30)):
        x = (rng.standard_normal(n) * scale).astype(np.float32)
        tp, bad = true_peak_model(x)
        assert bad == 0 and 0 < tp <= TAP_SUM * float(np.abs(x).max()) * ROUNDING, (n, scale)
    x = rng.choice(np.array([-1.0, 1.0], np.float32), 200000)      # signs find the bound's neighbourhood
    assert 1.5 < true_peak_model(x)[0] <= TAP_SUM


# ---- grail_true_peak_limit_gains --------------------------------------------------------------------------------------------
def test_limit_gains_at_and_one_step_above_the_ceiling(built):
    tp = np.array([0.5, 0.25, 0.0, 3.0], np.float64)
    above = np.nextafter(np.float32(2.0), np.float32(4.0))
    rows = np.array([0, 0, 0, 2, 1, 3, 3], np.uint32)
    gains = np.array([2.0, above, -above, 1e30, -4.0, 0.1, -5.0], np.float32)
    got, limited = G.true_peak_limit_gains(tp, rows, gains, 0.0)            # c = 1.0
    # exactly at the ceiling (2.0 x 0.5, -4.0 x 0.25): untouched; one unit in the last place above: limited, the sign kept;
    # a row of true peak 0: untouched whatever the gain; 1 / 3 rounds up in binary32, so the limit steps one float back
    third = np.float32(1.0 / 3.0)
    assert float(third) * 3.0 > 1.0
    want = np.array([2.0, 2.0, -2.0, 1e30, -4.0, 0.1, -np.nextafter(third, np.float32(0.0))], np.float32)
    assert same_bits(got, want) and limited == 3, (got, limited)
    model, model_limited = limit_model(tp, rows, gains, 0.0)
    assert same_bits(model, want) and model_limited == 3
    on = tp[rows] > 0
    assert np.all(np.abs(got[on]).astype(np.float64) * tp[rows][on] <= 1.0)


@pytest.mark.parametrize("ceiling_db", [-1.0, 0.0, -23.5, 6.0, -120.0])
def test_limit_gains_equal_the_model(built, ceiling_db):
    rng = np.random.default_rng(11)
    n_rows, n_items = 300, 5000
    tp = 10.0 ** rng.uniform(-3.0, 1.0, n_rows)
    tp[rng.integers(0, n_rows, 20)] = 0.0
    rows = rng.integers(0, n_rows, n_items).astype(np.uint32)
    c = ceiling_of(ceiling_db)
    with np.errstate(divide="ignore"):
        gains = (c / tp[rows] * 10.0 ** rng.uniform(-0.5, 0.5, n_items)).astype(np.float32)
    gains[~np.isfinite(gains)] = 1.0
    gains[::2] = -gains[::2]
    at = rng.integers(0, n_items, 500)                                      # right at the rounding of c / tp, either side
    with np.errstate(divide="ignore"):
        edge = (c / tp[rows[at]]).astype(np.float32)
    edge = np.where(np.isfinite(edge), edge, np.float32(1.0))
    gains[at] = np.where(rng.random(500) < 0.5, edge, np.nextafter(edge, np.float32(np.inf))).astype(np.float32)
    got, limited = G.true_peak_limit_gains(tp, rows, gains, ceiling_db)
    want, want_limited = limit_model(tp, rows, gains, ceiling_db)
    assert same_bits(got, want) and limited == want_limited and 0 < limited < n_items
    # what the rule is for: exact, so it is asserted
    assert np.all(np.abs(got).astype(np.float64) * tp[rows] <= c)
    assert np.array_equal(np.signbit(got), np.signbit(gains))
    changed = ~(got.view(np.uint32) == gains.view(np.uint32))
    assert np.count_nonzero(changed) <= limited                             # (a limited gain may equal what it was)
    assert same_bits(got[tp[rows] == 0], gains[tp[rows] == 0])


def test_limit_gains_invalid_arguments_leave_the_outputs_untouched(built):
    lib = G.load()
    tp = np.array([1.0, 2.0], np.float64)
    rows = np.array([0, 1, 1], np.uint32)
    bad_rows = np.array([0, 1, 2], np.uint32)
    for t, r, ceiling, with_gains in ((tp, bad_rows, 0.0, True), (None, rows, 0.0, True), (tp, None, 0.0, True),
                                      (tp, rows, 0.0, False), (tp, rows, float("nan"), True), (tp, rows, float("inf"), True),
                                      (tp, rows, float("-inf"), True)):
        g = np.full(3, 100.0, np.float32)
        n = C.c_uint32(99)
        rc = lib.grail_true_peak_limit_gains(None if t is None else t.ctypes.data, 2, None if r is None else r.ctypes.data, 3,
                                             ceiling, g.ctypes.data if with_gains else None, C.addressof(n))
        assert rc == G.ERR_INVALID_ARG and np.all(g == 100.0) and n.value == 99, (r, ceiling)
    # nothing to do is no error, and the count may be NULL
    n = C.c_uint32(99)
    assert lib.grail_true_peak_limit_gains(None, 0, None, 0, 0.0, None, C.addressof(n)) == G.OK and n.value == 0
    g = np.full(3, 100.0, np.float32)
    assert lib.grail_true_peak_limit_gains(tp.ctypes.data, 2, rows.ctypes.data, 3, 0.0, g.ctypes.data, None) == G.OK
    assert np.array_equal(g, np.array([1.0, 0.5, 0.5], np.float32))
    with pytest.raises(G.GrailError):
        G.true_peak_limit_gains(tp, bad_rows, [1.0, 1.0, 1.0], 0.0)


# ---- grail_true_peak_db -----------------------------------------------------------------------------------------------------
def test_true_peak_db(built):
    assert G.true_peak_db(1.0) == 0.0 and G.true_peak_db(0.0) == -math.inf
    for x in (7964.0 / 8192.0, 0.5, 1e-300, 2.02 * float(FLT_MAX), 10.0 ** (-1.0 / 20.0)):
        assert G.true_peak_db(x) == 20.0 * math.log10(x), x
    assert abs(G.true_peak_db(10.0 ** (-1.0 / 20.0)) + 1.0) <= 1e-12
    assert math.isnan(G.true_peak_db(float("nan"))) and math.isnan(G.true_peak_db(-1.0)) and math.isnan(G.true_peak_db(-math.inf))
    assert G.true_peak_db(-0.0) == -math.inf and G.true_peak_db(math.inf) == math.inf


# ---- signatures, and the device entry points without a device ---------------------------------------------------------------
def test_signatures_load_and_the_device_calls_fail_loudly_without_a_device(built):
    lib = G.load()
    for name in ("grail_true_peak_coefficients", "grail_true_peak_async", "grail_true_peak_db",
                 "grail_true_peak_limit_gains", "grail_batch_mix_leveled_limited"):
        assert name in G.EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.grail_true_peak_async.argtypes) == 7 and len(lib.grail_true_peak_limit_gains.argtypes) == 7
    assert len(lib.grail_batch_mix_leveled_limited.argtypes) == len(lib.grail_batch_mix_leveled.argtypes) + 2 == 18
    assert lib.grail_true_peak_db.restype is C.c_double
    assert lib.grail_abi_version() == 4                                     # additive: the version stays
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "levels, continued: true peak (ITU-R BS.1770-4 Annex 2)" in hdr
    if G.device_count() == 0:        # no context can exist: the calls say why, they do not compute on the CPU
        assert lib.grail_true_peak_async(None, None, 64, None, 1, None, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_batch_mix_leveled_limited(None, None, None, None, None, None, G.LEVEL_LOUDNESS, 0, None, 0, 0, 0,
                                                   None, None, None, -1.0, None, 0) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()


def test_dialogue_example_knows_the_ceiling_option(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--ceiling DBTP" in r.stderr and "--lufs L" in r.stderr and "--level DB" in r.stderr
    r = subprocess.run([exe, "--lufs", "-23", "--ceiling", "loud", "a", "e"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run([exe, "--ceiling", "-1", "a", "e"], capture_output=True, text=True)      # a ceiling on no level
    assert r.returncode == 2 and "usage" in r.stderr
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--lufs", "-23", "--ceiling", "-1", "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr


# ---- the host functions under the sanitizers ------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_true_peak_helpers_under_asan_ubsan(tmp_path):
    """csrc/level_gains.cpp makes no HIP call: built with g++ and the sanitizers, then driven by
    tests/sanitize_true_peak_driver.cpp over arrays of exactly the documented sizes."""
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-ffp-contract=off", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "level_gains.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_true_peak_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_true_peak_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize true peak driver: ok" in r.stdout
