"""The segmented K-weighting and what a meter reads from the hop sums, without a GPU (include/grail_hip.h, "levels,
continued": THE SEGMENTED FORM, grail_loudness_window_max, grail_loudness_range).

The numpy model of the segmented contract, segmented_hops_model(), on top of tests/test_loudness_host.py's
kweight_hops_model(): bit-equal to the serial model where the header says so, close to it everywhere else (measured, then
asserted with a margin), and the header's derived truncation bound evaluated.  grail_loudness_window_max and
grail_loudness_range bit for bit against numpy, and the range against the known answers of EBU Tech 3342.  Signatures, the
device entry point failing loudly without a device, and the new host functions under AddressSanitizer + UBSan through a
stand-alone driver (tests/sanitize_loudness_range_driver.cpp).  tests/test_loudness_segmented_gpu.py compares the device
with segmented_hops_model()."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import grail_hip as G
from test_levels_host import within_one_ulp
from test_loudness_host import (ABS_GATE, _clean, gate_model, kweight_hops_model, kweighting_model, lufs_model, same_bits,
                                tone)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 3                                        # GRAIL_LOUDNESS_WARMUP_HOPS, typed again

# How far the segmented model lies from the serial one over closeness_signals() (8 kHz, 30 hops and a ragged tail), as
# measured by test_the_segmented_model_is_close_to_the_serial_one when it was written:
#   largest |d hop| / H = MEASURED_HOP, largest |d LUFS| = MEASURED_LU   (P = 3)
# and what is asserted, here and of the device (tests/test_loudness_segmented_gpu.py): 100 times that, for signals not
# tried.  The header's truncation bound (2^-60 of the state) is far below either: what is measured is rounding noise.
MEASURED_HOP, MEASURED_LU = 6.2e-15, 1.8e-15      # (P = 2 gave 6.1e-15 and 2.7e-14 LU, P = 1 3.1e-11 and 5.2e-10 LU)
HOP_BOUND, LU_BOUND = 100 * MEASURED_HOP, 100 * MEASURED_LU


# ---- the segmented contract in numpy -----------------------------------------------------------------------------------
def segmented_hops_model(rows, rate, coef):
    """[(hop sums float64 [len // H], nonfinite)] per row, as grail_loudness_segmented_async defines them: hops 0 .. P-1
    from the serial model over the row's first P hops; for h >= P the slice x[(h-P) H : (h+1) H] run as a row of its own
    (from a zero state) and its last hop taken; the count over the whole row."""
    H = int(rate) // 10
    out = []
    for x in rows:
        x = np.asarray(x, np.float32)
        n_hops = len(x) // H
        head = kweight_hops_model([x[:min(n_hops, P) * H]], rate, coef)[0][0]
        slices = [x[(h - P) * H:(h + 1) * H] for h in range(P, n_hops)]
        rest = [hops[-1] for hops, _ in kweight_hops_model(slices, rate, coef)] if slices else []
        out.append((np.concatenate([head, np.array(rest, np.float64)]), _clean(x)[1]))
    return out


def window_blocks(hops, H, window):
    """the mean squares of the windows of `window` hops, one every hop: each a left fold from h[j] in ascending order,
    divided by (double)window * (double)H"""
    h = np.asarray(hops, np.float64)
    blocks = len(h) - window + 1
    if window == 0 or blocks <= 0:
        return np.zeros(0)
    s = h[:blocks].copy()
    for i in range(1, window):
        s = s + h[i:i + blocks]
    return s / (np.float64(window) * np.float64(H))


def window_max_model(hops, H, window):
    z = window_blocks(hops, H, window)
    best = np.float64(0.0)
    for v in z:
        if v > best:
            best = v
    return best


def range_model(hops, H):
    """(LU, |B|) after the header: blocks of 30 hops, the absolute gate, the relative gate 20 LU below the mean of what
    passed the absolute one, the 10th and the 95th percentile by Tech 3342's rounding"""
    s = window_blocks(hops, H, 30)
    if len(s) == 0:
        return 0.0, 0
    A = s[s > ABS_GATE]
    if len(A) == 0:
        return 0.0, 0
    total = np.float64(0.0)
    for v in A:
        total = total + v
    r = np.float64(0.01) * (total / np.float64(len(A)))
    B = np.sort(A[A > r])
    n = len(B)
    lo, hi = B[((n - 1) * 10 + 50) // 100], B[((n - 1) * 95 + 50) // 100]
    return 10.0 * math.log10(hi / lo), n


def one_ulp64(a, b):
    """binary64 values at most one unit in the last place apart (log10 is the C library's on one side)"""
    a, b = np.float64(a), np.float64(b)
    if a == b:
        return True
    return bool(abs(int(a.view(np.int64)) - int(b.view(np.int64))) <= 1) and within_one_ulp(np.float32(a), np.float32(b))


def truncation_bound(coef, H):
    """the header's D: |dz| <= D * (|s1| + |s2| + |s3| + |s4|), P * H samples after a start from zero"""
    rho, r = math.sqrt(coef[4]), math.sqrt(coef[9])
    assert coef[3] ** 2 < 4 * coef[4] and coef[8] ** 2 < 4 * coef[9] and rho < r < 1      # complex poles, the shelf's inside
    m = P * H
    return (m + 1) * r ** (m - 2) * (1.0 + 4.0 / (rho * (1.0 - rho / r) ** 2))


def closeness_signals(rate=8000, hops=30):
    """noise; DC plus a 50 Hz tone; a loud 30 Hz square, then digital silence; noise bursts — each of `hops` hops and a
    ragged tail"""
    H = rate // 10
    rng = np.random.default_rng(2024)
    n = hops * H + 137
    t = np.arange(n, dtype=np.float64)
    noise = (0.25 * rng.standard_normal(n)).astype(np.float32)
    dc_tone = (0.3 + 0.4 * np.sin(2.0 * np.pi * 50.0 * t / rate)).astype(np.float32)
    square = (0.9 * np.sign(np.sin(2.0 * np.pi * 30.0 * t / rate))).astype(np.float32)
    square[hops // 2 * H + 61:] = 0.0
    bursts = (0.5 * rng.standard_normal(n)).astype(np.float32)
    bursts[(np.arange(n) // (3 * H // 2)) % 2 == 1] = 0.0
    return {"noise": noise, "dc + 50 Hz": dc_tone, "square, then silence": square, "bursts": bursts}


# ---- the model against the serial model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [2570, 8000])
def test_hops_up_to_the_warm_up_equal_the_serial_model_bit_for_bit(rate):
    """hops 0 .. P are the serial hops; a row of 0, 1, P and P + 1 hops equals the serial model entirely (a tail or not)"""
    H = rate // 10
    rng = np.random.default_rng(rate)
    coef = kweighting_model(48000 if rate < 3364 else rate)
    lengths = [0, H - 1, H, H + 5, P * H, P * H + H - 1, (P + 1) * H, (P + 1) * H + 1, (P + 2) * H, 9 * H + 3]
    rows = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    rows[5][2 * H + 1] = np.nan
    rows[9][7] = np.inf
    serial, seg = kweight_hops_model(rows, rate, coef), segmented_hops_model(rows, rate, coef)
    for n, (hs, bs), (hg, bg) in zip(lengths, serial, seg):
        assert len(hg) == len(hs) == n // H and bs == bg
        assert same_bits(hg[:P + 1], hs[:P + 1]), n
        if n // H <= P + 1:
            assert same_bits(hg, hs) and same_bits(gate_model(hg, H), gate_model(hs, H))
    assert seg[5][1] == 1 and seg[9][1] == 1
    # ... and the later hops are the serial ones only nearly (at 2 570 Hz with the 48 kHz coefficients: not even nearly)
    if rate == 2570:
        assert not same_bits(seg[9][0], serial[9][0])


def test_the_segmented_model_is_close_to_the_serial_one():
    """K-weighting at 8 kHz, four kinds of signal: the largest |d hop| / H and |d LUFS| between the two models.
    Measured when written (P = 3): see MEASURED_HOP, MEASURED_LU above; asserted: 100 times that."""
    rate, H = 8000, 800
    coef = kweighting_model(rate)
    worst_hop = worst_lu = 0.0
    for name, x in closeness_signals(rate).items():
        (hs, _), = kweight_hops_model([x], rate, coef)
        (hg, _), = segmented_hops_model([x], rate, coef)
        d_hop = float(np.max(np.abs(hg - hs)) / H)
        ls, lg = lufs_model(gate_model(hs, H)), lufs_model(gate_model(hg, H))
        d_lu = abs(ls - lg)
        equal = int(np.count_nonzero(hg.view(np.uint64) == hs.view(np.uint64)))
        print(f"\n{name}: |d hop| / H {d_hop:.2e}, |d LUFS| {d_lu:.2e} at {ls:.3f} LUFS, {equal} of {len(hs)} hops bit-equal")
        assert len(hs) == 30 and np.isfinite(ls)
        worst_hop, worst_lu = max(worst_hop, d_hop), max(worst_lu, d_lu)
    print(f"largest: {worst_hop:.2e} (asserted {HOP_BOUND:.1e}), {worst_lu:.2e} LU (asserted {LU_BOUND:.1e})")
    assert worst_hop <= HOP_BOUND and worst_lu <= LU_BOUND


def test_the_headers_truncation_bound_lies_below_two_to_the_minus_60(built):
    for rate in (8000, 44100, 48000, 192000):
        for coef in (kweighting_model(rate), G.kweighting(rate)):
            H = rate // 10
            D = truncation_bound(coef, H)
            r_hop = math.sqrt(coef[9]) ** H
            print(f"\n{rate} Hz: r^H {r_hop:.3e}, D {D:.2e}")
            assert 3.9e-11 < r_hop < 4.0e-11                # a time constant in seconds: the same at every rate
            assert D < 2.0 ** -60


# ---- grail_loudness_window_max, grail_loudness_range -----------------------------------------------------------------
def _random_hops(rng, n, H, quiet=()):
    h = rng.uniform(0.2, 1.0, n) * H * 10.0 ** rng.uniform(-3, -1)
    for i in quiet:
        h[i] *= 1e-9
    return h


def test_window_max_and_range_equal_the_model(built):
    rng = np.random.default_rng(31)
    H = 4800
    for n in (0, 1, 3, 4, 5, 29, 30, 31, 400):
        for trial in range(3):
            h = _random_hops(rng, n, H)
            if trial == 1 and n:
                h[rng.random(n) < 0.5] *= 1e-6             # stretches 60 dB down: the relative gate cuts
            if trial == 2 and n:
                h[rng.random(n) < 0.7] = 0.0
            for w in (4, 30, 1, 7):
                assert same_bits(G.loudness_window_max(h, H, w), window_max_model(h, H, w)), (n, w)
            got, (want, _) = G.loudness_range(h, H), range_model(h, H)
            assert one_ulp64(got, want), (n, trial, got, want)
            assert (got == 0.0) if n < 31 else (got >= 0.0)             # (30 hops are one block: hi == lo)
            assert not (n == 400 and trial == 0) or got > 0.0
            if n >= 4:                                      # for window 4 the blocks are the gate's
                z = window_blocks(h, H, 4)
                assert same_bits(z, (((h[:-3] + h[1:-2]) + h[2:-1]) + h[3:]) / np.float64(4.0 * H))
    h = _random_hops(rng, 40, H)
    lib = G.load()
    assert G.loudness_window_max(h, H, 0) == 0.0 and G.loudness_window_max(h, 0, 4) == 0.0
    assert G.loudness_window_max(h, H, 41) == 0.0 and G.loudness_window_max(h, H, 40) > 0.0
    assert lib.grail_loudness_window_max(None, 40, H, 4) == 0.0 and lib.grail_loudness_range(None, 40, H) == 0.0
    assert G.loudness_range(h, 0) == 0.0 and G.loudness_range(h[:29], H) == 0.0


def test_range_of_everything_below_the_absolute_gate_is_zero(built):
    H = 4800
    h = np.full(100, ABS_GATE * H * 0.999)
    assert G.loudness_range(h, H) == 0.0 and range_model(h, H) == (0.0, 0)
    assert same_bits(G.loudness_window_max(h, H, 30), window_max_model(h, H, 30)) and 0 < G.loudness_window_max(h, H, 30) < ABS_GATE


def _hop_for_block(target, per):
    """a hop sum c with c / per == target exactly (a lone hop among zeros is its window's whole sum)"""
    c = np.float64(target) * per
    for _ in range(4):
        c = np.nextafter(c, 0.0)
    for _ in range(9):
        if c / per == target:
            return c
        c = np.nextafter(c, np.inf)
    raise AssertionError("no hop sum gives the block exactly")


def test_range_one_unit_in_the_last_place_either_side_of_both_thresholds(built):
    """31 hops, all zero but the first and the last: two blocks, the first hop's and the last's, each a lone hop / (30 H).
    H = 4370 makes 30 H = 2^17 * 1.0002: a hop sum c = q * 30 H then lies in a binade where consecutive c give quotients
    less than one unit in the last place of q apart, so every q below is some c / (30 H) exactly."""
    H = 4370
    per = np.float64(30.0) * np.float64(H)
    up, down = np.nextafter(ABS_GATE, 1.0), np.nextafter(ABS_GATE, 0.0)
    for q, passes in ((up, True), (ABS_GATE, False), (down, False)):
        h = np.zeros(31)
        h[0], h[30] = _hop_for_block(q, per), _hop_for_block(10.0 * ABS_GATE, per)
        assert same_bits(window_blocks(h, H, 30), [q, 10.0 * ABS_GATE])
        got, (want, nb) = G.loudness_range(h, H), range_model(h, H)
        assert one_ulp64(got, want) and nb == (2 if passes else 1), (q, got, want)
        assert (abs(got - 10.0) < 1e-9) if passes else (got == 0.0)
    # the relative gate: blocks [q, 298.5]: r = 0.01 * ((q + 298.5) / 2) is 1.5 exactly for q = 1.5 and one ulp either side
    for q, kept in ((np.float64(1.5), False), (np.nextafter(1.5, 0.0), False), (np.nextafter(1.5, 2.0), True)):
        h = np.zeros(31)
        h[0], h[30] = _hop_for_block(q, per), _hop_for_block(298.5, per)
        assert same_bits(window_blocks(h, H, 30), [q, 298.5])
        assert np.float64(0.01) * ((np.float64(0.0) + q + np.float64(298.5)) / np.float64(2.0)) == 1.5
        got, (want, nb) = G.loudness_range(h, H), range_model(h, H)
        assert one_ulp64(got, want) and nb == (2 if kept else 1), (q, got, want)
        assert (abs(got - 10.0 * math.log10(199.0)) < 1e-9) if kept else (got == 0.0)


@pytest.mark.parametrize("size", [1, 2, 10, 11, 21])
def test_range_percentiles_step_with_the_number_of_blocks(built, size):
    """|B| = 1, 2, 10, 11, 21: the indices ((|B|-1) * 10 + 50) / 100 and ((|B|-1) * 95 + 50) / 100 are 0 0 1 1 2 and
    0 1 9 10 19"""
    H = 4410
    rng = np.random.default_rng(size)
    h = rng.uniform(0.5, 1.0, 29 + size) * H * rng.uniform(0.01, 1.0, 29 + size)
    got, (want, nb) = G.loudness_range(h, H), range_model(h, H)
    assert nb == size and one_ulp64(got, want), (got, want)
    B = np.sort(window_blocks(h, H, 30))
    lo = {1: 0, 2: 0, 10: 1, 11: 1, 21: 2}[size]
    hi = {1: 0, 2: 1, 10: 9, 11: 10, 21: 19}[size]
    assert len(np.unique(B)) == size and one_ulp64(got, 10.0 * math.log10(B[hi] / B[lo]))


def test_range_reads_the_known_answers_of_tech_3342(built):
    """EBU Tech 3342's test signals, scaled to 8 kHz: a 1 kHz tone in sections of 20 s, through the serial model and
    grail_loudness_range: 10, 5, 20 and 15 LU within the standard's +-1 LU.  (The definition gives 10.0000003, 4.9999997,
    20.0000005 and 15.0000001.)"""
    rate, H = 8000, 800
    coef = kweighting_model(rate)
    cases = (((-20, -30), 10.0), ((-20, -15), 5.0), ((-40, -20), 20.0), ((-50, -35, -20, -35, -50), 15.0))
    rows = [np.concatenate([tone(rate, 20.0, db, hz=1000.0, start=k * 20 * rate) for k, db in enumerate(levels)])
            for levels, _ in cases]
    for (levels, want), (hops, _) in zip(cases, kweight_hops_model(rows, rate, coef)):
        got = G.loudness_range(hops, H)
        print(f"\n{levels} dBFS: {got:.7f} LU")
        assert abs(got - want) <= 1.0
        assert abs(got - want) <= 1e-5          # (what the definition gives, to the digits above)
        assert one_ulp64(got, range_model(hops, H)[0])


# ---- signatures, and the device entry point without a device --------------------------------------------------------------
def test_signatures_load_and_the_device_call_fails_loudly_without_a_device(built):
    lib = G.load()
    for name in ("grail_loudness_segmented_async", "grail_loudness_window_max", "grail_loudness_range"):
        assert name in G.EXPORTS and getattr(lib, name).argtypes is not None
    assert lib.grail_loudness_segmented_async.argtypes == lib.grail_loudness_async.argtypes
    assert len(lib.grail_loudness_window_max.argtypes) == 4 and len(lib.grail_loudness_range.argtypes) == 3
    assert lib.grail_loudness_window_max.restype is C.c_double and lib.grail_loudness_range.restype is C.c_double
    assert G.LOUDNESS_WARMUP_HOPS == P and hasattr(G.Context, "loudness_segmented") and hasattr(G.Context, "loudness_segmented_async")
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    assert "#define GRAIL_LOUDNESS_WARMUP_HOPS 3u" in hdr
    assert re_abi(hdr) == "4"
    if G.device_count() == 0:        # no context can exist: the call says why, it does not compute on the CPU
        assert lib.grail_loudness_segmented_async(None, None, 64, None, 1, 48000, None, None, None, 0, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error()


def re_abi(hdr):
    import re
    return re.search(r"#define GRAIL_ABI_VERSION (\d+)", hdr).group(1)


def test_dialogue_example_knows_the_report_option(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "[--report]" in r.stderr
    for misuse in (["--report=yes", "a", "e"], ["--report", "--report", "a", "e"], ["--report", "a"]):
        r = subprocess.run([exe] + misuse, capture_output=True, text=True)
        assert r.returncode == 2 and "usage" in r.stderr, misuse
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--report", "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr


# ---- the new host functions under the sanitizers ------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_range_and_window_max_under_asan_ubsan(tmp_path):
    """csrc/level_gains.cpp makes no HIP call: built with g++ and the sanitizers, then driven by the stand-alone
    tests/sanitize_loudness_range_driver.cpp over arrays of exactly n_hops entries."""
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-ffp-contract=off", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "level_gains.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_loudness_range_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_loudness_range_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize loudness range driver: ok" in r.stdout
