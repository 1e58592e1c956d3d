"""K-weighted gated loudness without a GPU (include/grail_hip.h, "levels, continued"): grail_kweighting against the same
formulas in numpy and against the table BS.1770 prints for 48 kHz, grail_gated_mean_square bit for bit against the gate
written in numpy, grail_level_gains in GRAIL_LEVEL_LOUDNESS, the ctypes signatures, the device entry point failing loudly
without a device, and the pure-host functions built with g++ under AddressSanitizer + UBSan and driven by
tests/sanitize_loudness_driver.cpp.

Also the numpy model of the contract, written from the header's words, that tests/test_loudness_gpu.py compares the device
with: kweight_hops_model() and gate_model() — and that model against the standard's calibration points, so that the
contract is BS.1770 and not merely consistent with itself."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import grail_hip as G
from test_levels_host import gains_model, within_one_ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.float32(3.4028234663852886e38)
ABS_GATE = 1.1724653045822981e-07            # the header's literal, typed again: 10^((-70 + 0.691) / 10)
LEVEL_SCALE = 0.8529037030705663             # 10^(-0.691 / 10)
RATES = (8000, 16000, 22050, 44100, 48000, 96000, 192000)
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, then of the high-pass
BS1770_48K = np.array([1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                       1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621])


# ---- the contract in numpy -------------------------------------------------------------------------------------------
def kweighting_model(rate):
    """the header's formulas, in the header's order of operations"""
    out = np.zeros(10)
    K, Q = np.tan(np.pi * 1681.974450955533 / rate), 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    out[:5] = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
               2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    K, Q = np.tan(np.pi * 38.13547087602444 / rate), 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    out[5:] = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return out


def _clean(x):
    """(the samples as binary64 with +0.0 in place of the non-finite ones, the count of those)"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        finite = np.abs(x) <= FLT_MAX
    return np.where(finite, x, np.float32(0.0)).astype(np.float64), int(np.count_nonzero(~finite))


def _hops_of_one_row(x, H, coef):
    """One row in Python floats (IEEE binary64, every operation rounded by itself, exactly like numpy's float64 — and an
    order of magnitude faster than numpy on arrays of one element)."""
    v_all, bad = _clean(x)
    b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = (float(c) for c in coef)
    s1 = s2 = s3 = s4 = 0.0
    hops = []
    n_hops = len(v_all) // H
    for h in range(n_hops):
        acc = 0.0
        for v in v_all[h * H:(h + 1) * H].tolist():
            y = b0 * v + s1
            s1 = (b1 * v - a1 * y) + s2
            s2 = b2 * v - a2 * y
            z = d0 * y + s3
            s3 = (d1 * y - e1 * z) + s4
            s4 = d2 * y - e2 * z
            acc = acc + z * z
        hops.append(acc)
    return np.array(hops, np.float64), bad          # (the samples after the last whole hop belong to no hop)


def kweight_hops_model(rows, rate, coef):
    """[(hop sums float64 [len // H], nonfinite)] for rows (a list of float32 arrays of any lengths) at `rate`.
    coef: float64 [10], or [len(rows)][10] for coefficients per row.  The two biquads in transposed direct form II, the
    sum of z*z per hop of H = rate // 10 samples, as the header writes them.  Many rows are run vectorised across rows
    with a Python loop over t; a few rows one after the other in Python floats: the same operations in the same order."""
    H = int(rate) // 10
    rows = [np.asarray(x, np.float32) for x in rows]
    coef = np.asarray(coef, np.float64)
    per_row = np.broadcast_to(coef, (len(rows), 10))
    if len(rows) < 16:
        return [_hops_of_one_row(x, H, per_row[i]) for i, x in enumerate(rows)]
    return _hops_vectorised(rows, H, per_row)


def _hops_vectorised(rows, H, per_row):
    order = sorted(range(len(rows)), key=lambda i: -len(rows[i]))          # longest first: the live rows are a prefix
    lens = np.array([len(rows[i]) for i in order])
    longest = int(lens[0]) if len(lens) else 0
    v = np.zeros((len(rows), max(longest, 1)), np.float64)
    bad = []
    for k, i in enumerate(order):
        v[k, :lens[k]], b = _clean(rows[i])
        bad.append(b)
    c = np.ascontiguousarray(per_row[order].T)                              # c[j] = coefficient j of every row
    s1, s2, s3, s4, acc = (np.zeros(len(rows)) for _ in range(5))
    hops = np.zeros((len(rows), max(longest // H, 1)), np.float64)
    vt = np.ascontiguousarray(v.T)
    for h in range(longest // H):
        k = int(np.count_nonzero(lens >= (h + 1) * H))                      # the rows that hold this whole hop: a prefix
        acc[:k] = 0.0
        for t in range(h * H, (h + 1) * H):
            x = vt[t, :k]
            y = c[0, :k] * x + s1[:k]
            s1[:k] = (c[1, :k] * x - c[3, :k] * y) + s2[:k]
            s2[:k] = c[2, :k] * x - c[4, :k] * y
            z = c[5, :k] * y + s3[:k]
            s3[:k] = (c[6, :k] * y - c[8, :k] * z) + s4[:k]
            s4[:k] = c[7, :k] * y - c[9, :k] * z
            acc[:k] = acc[:k] + z * z
        hops[:k, h] = acc[:k]
    out = [None] * len(rows)
    for k, i in enumerate(order):
        out[i] = (hops[k, :lens[k] // H].copy(), bad[k])
    return out


def gate_model(hops, H):
    """the gated mean square of one row's hop sums: blocks of four hops every hop, the absolute gate, the relative gate at
    0.1 of the mean of what passed the absolute one; every sum a left fold from +0.0 in ascending order"""
    h = np.asarray(hops, np.float64)
    if len(h) < 4:
        return np.float64(0.0)
    z = (((h[:-3] + h[1:-2]) + h[2:-1]) + h[3:]) / np.float64(4.0 * H)

    def mean(sel):
        s = np.float64(0.0)
        for v in z[sel]:
            s = s + v
        return s / np.float64(np.count_nonzero(sel))

    with np.errstate(invalid="ignore"):
        A = z > ABS_GATE
        if not A.any():
            return np.float64(0.0)
        r = np.float64(0.1) * mean(A)
        B = A & (z > r)
    return mean(B) if B.any() else np.float64(0.0)


def lufs_model(ms):
    return -0.691 + 10.0 * np.log10(ms) if ms > 0 else -np.inf


def loudness_model(x, rate, coef=None):
    """LUFS of one row by the model"""
    coef = kweighting_model(rate) if coef is None else coef
    hops, _ = kweight_hops_model([x], rate, coef)[0]
    return lufs_model(gate_model(hops, rate // 10))


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def tone(rate, seconds, dbfs, hz=997.0, start=0):
    t = np.arange(start, start + int(round(rate * seconds)), dtype=np.float64)
    return (10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * hz * t / rate)).astype(np.float32)


# ---- the model against the standard -------------------------------------------------------------------------------------
def test_the_model_reads_the_standards_calibration_tone(built):
    """BS.1770: a 997 Hz sine at full scale reads -3.01 LKFS; the same 20 dB down, -23.01.  With grail_kweighting(48000)."""
    coef = G.kweighting(48000)
    for dbfs, want in ((0.0, -3.01), (-20.0, -23.01)):
        got = loudness_model(tone(48000, 3.0, dbfs), 48000, coef)
        print(f"\n997 Hz at {dbfs} dBFS: {got:.4f} LUFS")
        assert abs(got - want) <= 0.05


def test_the_two_forms_of_the_model_agree_bit_for_bit():
    rng = np.random.default_rng(5)
    rows = [rng.standard_normal(n).astype(np.float32) for n in (0, 1, 255, 256, 1024, 1025, 1500, 2049)] * 2
    rows[3][7] = np.nan
    rows[4][100] = np.float32(-0.0)
    coef = kweighting_model(8000)              # (hops of 256 samples all the same: the hop length is the caller's)
    a = _hops_vectorised(rows, 256, np.broadcast_to(coef, (16, 10)))
    for x, (hops, bad) in zip(rows, a):
        h1, b1 = _hops_of_one_row(x, 256, coef)
        assert same_bits(hops, h1) and bad == b1 and len(hops) == len(x) // 256
    assert a[3][1] == 1


def test_the_relative_gate_discards_the_quiet_parts(built):
    """EBU Tech 3341 case 3, scaled down: a tone 13 dB down, the tone, 13 dB down again.  The quiet parts lie more than
    10 LU below the mean of everything and are discarded: the figure is the tone's.  (The three blocks across each of
    the two steps stay in; with 30 s of tone they move the mean by 10 log10((297 + 3.1) / 303) = -0.04 LU.)"""
    rate = 8000
    alone = loudness_model(tone(rate, 30.0, -23.0), rate)
    x = np.concatenate([tone(rate, 2.0, -36.0), tone(rate, 30.0, -23.0, start=2 * rate), tone(rate, 2.0, -36.0, start=32 * rate)])
    got = loudness_model(x, rate)
    print(f"\nthe tone alone {alone:.4f} LUFS, between quiet parts {got:.4f} LUFS")
    assert abs(got - alone) <= 0.1
    # ... while without a gate the quiet four seconds would pull it down by 10 log10((30 + 4 * 0.05) / 34) = -0.5 LU
    hops, _ = kweight_hops_model([x], rate, kweighting_model(rate))[0]
    ungated = lufs_model(hops.sum() / len(x))
    assert ungated < alone - 0.4


def test_the_absolute_gate_discards_what_lies_below_minus_70(built):
    """a stretch at -80 dBFS before and after the tone must not move the figure: its blocks never pass the absolute gate,
    however long it is, and it reads as digital silence in the same places does"""
    rate = 8000
    body = tone(rate, 20.0, -23.0, start=4 * rate)
    floor = lambda s, at: tone(rate, s, -80.0, start=at)
    a = loudness_model(np.concatenate([floor(2.0, 2 * rate), body, floor(2.0, 24 * rate)]), rate)
    b = loudness_model(np.concatenate([floor(4.0, 0), body, floor(3.0, 24 * rate)]), rate)
    c = loudness_model(np.concatenate([np.zeros(2 * rate, np.float32), body, np.zeros(2 * rate, np.float32)]), rate)
    alone = loudness_model(body, rate)
    print(f"\n{a:.6f} {b:.6f} {c:.6f} alone {alone:.6f}")
    assert abs(a - b) < 1e-3 and abs(a - c) < 1e-3 and abs(a - alone) <= 0.1
    assert loudness_model(floor(3.0, 0), rate) == -np.inf           # nothing passes the gate: no loudness


# ---- grail_kweighting --------------------------------------------------------------------------------------------------
def test_kweighting_equals_the_formulas(built):
    for rate in RATES + (2560, 1048576):
        got, want = G.kweighting(rate), kweighting_model(rate)
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (rate, got, want)
    assert G.kweighting(48000)[5:8].tolist() == [1.0, -2.0, 1.0]


def test_kweighting_at_48k_is_the_standards_table(built):
    """The bilinear transform of the prototypes against the ten numbers BS.1770 prints (15 significant digits; the
    prototypes' constants were fitted to them).  Measured with numpy when this test was written: the largest relative
    difference is 3.3e-16 (the shelf's b1; b2 and the high-pass numerator are equal), far closer than the "about eight
    digits" that was expected.  Asserted: twice the measured value."""
    got = G.kweighting(48000)
    rel = np.abs(got - BS1770_48K) / np.abs(BS1770_48K)
    print(f"\nrelative differences from the table: {rel}")
    assert rel.max() <= 2 * 3.3e-16


def test_kweighting_refuses_rates_out_of_range(built):
    lib = G.load()
    for rate in (0, 1, 2559, 1048577, 0xFFFFFFFF):
        coef = np.full(10, 7.5)
        assert lib.grail_kweighting(rate, coef.ctypes.data) == G.ERR_INVALID_ARG
        assert np.all(coef == 7.5)
    assert lib.grail_kweighting(48000, None) == G.ERR_INVALID_ARG


# ---- grail_gated_mean_square --------------------------------------------------------------------------------------------
def test_gate_equals_the_model_bit_for_bit(built):
    rng = np.random.default_rng(11)
    H = 4800
    per = 4.0 * H
    cases = [rng.random(n) * per * 10.0 ** rng.uniform(-9, 0) for n in (4, 5, 7, 20, 61, 300) for _ in range(6)]
    # loud and quiet stretches, so that both gates cut
    for _ in range(20):
        n = int(rng.integers(4, 120))
        cases.append(rng.random(n) * per * 10.0 ** rng.choice([-9.0, -7.5, -4.0, -2.0, -1.0], n))
    # fewer than four hops: no block
    cases += [np.zeros(0), np.ones(1) * per, np.ones(3) * per]
    # every block under the absolute gate; exactly one over it
    cases.append(np.full(12, ABS_GATE * H * 0.99))
    one = np.full(12, ABS_GATE * H * 0.5)
    one[11] = ABS_GATE * H * 3.0
    cases.append(one)
    for hops in cases:
        got, want = G.gated_mean_square(hops, H), gate_model(hops, H)
        assert same_bits(got, want), (len(hops), got, want)
    assert G.gated_mean_square(cases[-2], H) == 0.0 and G.gated_mean_square(np.ones(3) * per, H) == 0.0
    assert G.gated_mean_square(one, H) == (one[8:12].sum()) / per and gate_model(one, H) > ABS_GATE


def test_gate_one_unit_in_the_last_place_either_side_of_both_thresholds(built):
    """H = 4096 makes 4 H a power of two: a block of four equal hops v * H has the mean square v exactly"""
    H = 4096
    up, down = np.nextafter(ABS_GATE, 1.0), np.nextafter(ABS_GATE, 0.0)
    for v, passes in ((up, True), (ABS_GATE, False), (down, False)):
        hops = np.full(4, v * H)
        assert same_bits(hops * 4, np.full(4, v * 4 * H))                       # (the scaling is exact)
        got = G.gated_mean_square(hops, H)
        assert same_bits(got, gate_model(hops, H)) and got == (v if passes else 0.0)
    # the relative gate: five hops [19 * 4H, 0, 0, 0, q * 4H] are two blocks, z = [19, q], both far above the absolute
    # gate; r = 0.1 * ((19 + q) / 2), which is 1.0 exactly for q = 1 and for q one ulp either side of it (19 + q rounds
    # to 20).  So q = 1 and the q below are not above r and leave block 0 alone; the q above 1 is kept.
    for q, kept in ((np.float64(1.0), False), (np.nextafter(1.0, 0.0), False), (np.nextafter(1.0, 2.0), True)):
        hops = np.array([19.0 * 4 * H, 0.0, 0.0, 0.0, q * 4 * H])
        got, want = G.gated_mean_square(hops, H), gate_model(hops, H)
        assert same_bits(got, want), (q, got, want)
        assert got == ((np.float64(19.0) + q) / 2.0 if kept else 19.0)


def test_lufs_and_level_formulas(built):
    assert G.loudness_lufs(0.0) == -np.inf
    for ms in (1e-9, ABS_GATE, 0.005, 0.5, 1.0, 3.7):
        assert abs(G.loudness_lufs(ms) - (-0.691 + 10.0 * math.log10(ms))) < 1e-12
        level = G.loudness_level(ms)
        assert level == math.sqrt(ms * LEVEL_SCALE)
        assert abs(20.0 * math.log10(level) - G.loudness_lufs(ms)) < 1e-9
    assert G.loudness_level(0.0) == 0.0
    assert abs(G.loudness_lufs(ABS_GATE) + 70.0) < 1e-9
    assert (G.LOUDNESS_ABS_GATE, G.LOUDNESS_LEVEL_SCALE) == (ABS_GATE, LEVEL_SCALE)
    assert ABS_GATE == 10.0 ** ((-70 + 0.691) / 10) and LEVEL_SCALE == 10.0 ** -0.0691


# ---- grail_level_gains in the new mode ----------------------------------------------------------------------------------
def test_level_gains_in_loudness_mode(built):
    rng = np.random.default_rng(3)
    n_rows, n_items = 40, 300
    ms = 10.0 ** rng.uniform(-7, 0, n_rows)
    ms[[0, 5]] = 0.0                                   # rows shorter than 400 ms, or gated out altogether
    bad = np.zeros(n_rows, np.uint32)
    bad[7] = 2
    level = np.array([G.loudness_level(m) for m in ms])
    rows = rng.integers(0, n_rows, n_items).astype(np.uint32)
    lufs = rng.uniform(-40, -10, n_items).astype(np.float32)
    got, out = G.level_gains(G.LEVEL_LOUDNESS, rows, lufs, nonfinite=bad, active_level=level)
    want, want_out = gains_model(G.LEVEL_LOUDNESS, lufs, rows, nonfinite=bad, active=level)
    assert within_one_ulp(got, want) and out == want_out == int(np.isin(rows, [0, 5, 7]).sum())
    assert np.all(got[np.isin(rows, [0, 5, 7])] == 0.0)
    # a row brought to its target reads the target: gain^2 * ms has the target's loudness
    k = int(np.flatnonzero(~np.isin(rows, [0, 5, 7]))[0])
    assert abs(G.loudness_lufs(float(got[k]) ** 2 * ms[rows[k]]) - float(lufs[k])) < 1e-5
    # the mode needs active_level; 3, 5 and 7 are still no modes
    lib = G.load()
    g = np.full(4, -1.0, np.float32)
    r4, db4 = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    lv = np.ones(3)
    assert lib.grail_level_gains(G.LEVEL_LOUDNESS, None, None, None, None, None, 3, r4.ctypes.data, db4.ctypes.data, 4,
                                 g.ctypes.data, None) == G.ERR_INVALID_ARG
    for mode in (3, 5, 7, -1):
        assert lib.grail_level_gains(mode, None, None, None, None, lv.ctypes.data, 3, r4.ctypes.data, db4.ctypes.data, 4,
                                     g.ctypes.data, None) == G.ERR_INVALID_ARG
    assert np.all(g == -1.0)
    assert lib.grail_level_gains(G.LEVEL_LOUDNESS, None, None, None, None, lv.ctypes.data, 3, r4.ctypes.data,
                                 db4.ctypes.data, 4, g.ctypes.data, None) == G.OK
    assert np.all(g == np.float32(1.0))


# ---- signatures, and the device entry point without a device --------------------------------------------------------------
def test_signatures_load_and_the_device_call_fails_loudly_without_a_device(built):
    lib = G.load()
    for name in ("grail_kweighting", "grail_loudness_async", "grail_gated_mean_square", "grail_loudness_lufs",
                 "grail_loudness_level"):
        assert name in G.EXPORTS and getattr(lib, name).argtypes is not None
    assert len(lib.grail_loudness_async.argtypes) == 11 and len(lib.grail_kweighting.argtypes) == 2
    assert len(lib.grail_gated_mean_square.argtypes) == 3
    for f in (lib.grail_gated_mean_square, lib.grail_loudness_lufs, lib.grail_loudness_level):
        assert f.restype is C.c_double
    assert G.LEVEL_LOUDNESS == 4 and G.LEVEL_LOUDNESS not in (G.LEVEL_PEAK, G.LEVEL_RMS, G.LEVEL_ACTIVE)
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    for text in ("#define GRAIL_LEVEL_LOUDNESS       4", "#define GRAIL_LOUDNESS_ABS_GATE    1.1724653045822981e-07",
                 "#define GRAIL_LOUDNESS_LEVEL_SCALE 0.8529037030705663", "#define GRAIL_ABI_VERSION"):
        assert text in hdr
    if G.device_count() == 0:        # no context can exist: the call says why, it does not compute on the CPU
        assert lib.grail_loudness_async(None, None, 64, None, 1, 48000, None, None, None, 0, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()
        assert lib.grail_batch_mix_leveled(None, None, None, None, None, None, G.LEVEL_LOUDNESS, 0, None, 0, 0, 0, None,
                                           None, None, 0) == G.ERR_NO_DEVICE


def test_dialogue_example_knows_the_lufs_option(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "--lufs L" in r.stderr and "--level DB" in r.stderr
    r = subprocess.run([exe, "--lufs", "loud", "a", "e"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--lufs", "-23", "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr


# ---- the host functions under the sanitizers ------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_loudness_helpers_under_asan_ubsan(tmp_path):
    """csrc/level_gains.cpp makes no HIP call: built with g++ and the sanitizers, then driven by
    tests/sanitize_loudness_driver.cpp over arrays of exactly the documented sizes."""
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-ffp-contract=off", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "level_gains.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_loudness_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_loudness_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize loudness driver: ok" in r.stdout
