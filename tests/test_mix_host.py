"""The host side of mixing, without a GPU: grail_mix_place_sequential against a restatement in Python,
grail_wav_write_i16_frames' RIFF header, the plan of grail_mix_async (csrc/mix_plan.cpp, no HIP) built with g++ under
AddressSanitizer + UBSan and driven by tests/sanitize_mix_driver.cpp, and the dialogue example failing loudly without a
device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import grail_hip as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def place(row_len, item_rows, item_tracks, gaps, n_tracks):
    """the header's rule: items on a track end to end in accumulation order (ascending row, ties as given); None: rejected"""
    n = len(item_rows)
    tracks = np.zeros(n, np.int64) if item_tracks is None else item_tracks
    gaps = np.zeros(n, np.int64) if gaps is None else gaps
    cursor, furthest, offs = [0] * n_tracks, [0] * n_tracks, [0] * n
    for i in sorted(range(n), key=lambda i: (int(item_rows[i]), i)):
        t = int(tracks[i])
        start = cursor[t] + int(gaps[i])
        if start < 0:
            return None
        offs[i] = start
        cursor[t] = start + int(row_len[item_rows[i]])
        furthest[t] = max(furthest[t], cursor[t])
    return np.array(offs, np.uint64), np.array(furthest, np.uint64)


@pytest.mark.parametrize("seed", range(16))
def test_sequential_placement_matches_a_restatement(built, seed):
    rng = np.random.default_rng(seed)
    n_rows, n_tracks = int(rng.integers(1, 40)), int(rng.integers(1, 7))
    row_len = rng.integers(0, 5000, n_rows).astype(np.uint32)
    row_len[rng.random(n_rows) < 0.1] = 0
    n_items = int(rng.integers(0, 90))
    item_rows = rng.integers(0, n_rows, n_items).astype(np.uint32)               # several items per row
    item_tracks = None if seed % 4 == 0 else rng.integers(0, max(1, n_tracks - 1), n_items).astype(np.uint32)  # an empty track
    gaps = None if seed % 3 == 0 else rng.integers(-300, 2500, n_items).astype(np.int64)
    if gaps is not None and seed % 2 == 0:
        gaps = np.abs(gaps)                                                      # no start below 0
    want = place(row_len, item_rows, item_tracks, gaps, n_tracks)
    if want is None:
        with pytest.raises(G.GrailError) as ei:
            G.mix_place_sequential(row_len, item_rows, item_tracks, gaps, n_tracks)
        assert ei.value.status == G.ERR_INVALID_ARG
        return
    offs, track_len = G.mix_place_sequential(row_len, item_rows, item_tracks, gaps, n_tracks)
    assert np.array_equal(offs, want[0]) and np.array_equal(track_len, want[1])
    if item_tracks is not None:
        assert track_len[n_tracks - 1] == 0 or n_tracks == 1


def test_negative_gaps_overlap_and_a_start_below_zero_is_rejected(built):
    row_len = np.array([100, 40], np.uint32)
    offs, tl = G.mix_place_sequential(row_len, [1, 0, 0], None, [-0, 10, -50], 1)
    # accumulation order: row 0 (item 1), row 0 (item 2), row 1 (item 0)
    assert offs.tolist() == [160, 10, 60] and tl.tolist() == [200]
    offs, tl = G.mix_place_sequential(row_len, [0, 1], None, [0, -90], 1)          # the second ends before the first
    assert offs.tolist() == [0, 10] and tl.tolist() == [100]
    for gaps in ([-1, 0], [50, -151]):
        with pytest.raises(G.GrailError) as ei:
            G.mix_place_sequential(row_len, [0, 1], None, gaps, 1)
        assert ei.value.status == G.ERR_INVALID_ARG
    for rows, tracks in (([2], None), ([0], [1])):                                # a row / track out of range
        with pytest.raises(G.GrailError):
            G.mix_place_sequential(row_len, rows, tracks, None, 1)


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_multichannel_wav_header_and_body(built, tmp_path, channels):
    rng = np.random.default_rng(channels)
    frames = rng.integers(-32768, 32768, (1001, channels)).astype(np.int16)
    path = str(tmp_path / "f.wav")
    G.wav_write_i16_frames(path, frames, 48000)
    data = open(path, "rb").read()
    n = frames.size * 2
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == 36 + n and data[8:16] == b"WAVEfmt "
    sub, fmt, ch, rate, byte_rate, align, bits = struct.unpack("<IHHIIHH", data[16:36])
    assert (sub, fmt, ch, rate, bits) == (16, 1, channels, 48000, 16)
    assert byte_rate == 48000 * 2 * channels and align == 2 * channels
    assert data[36:40] == b"data" and struct.unpack("<I", data[40:44])[0] == n
    assert data[44:] == frames.astype("<i2").tobytes() and len(data) == 44 + n


def test_one_channel_is_byte_identical_to_the_mono_writer(built, tmp_path):
    pcm = np.random.default_rng(3).integers(-32768, 32768, 777).astype(np.int16)
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    G.wav_write_i16(a, pcm, 44100)
    G.wav_write_i16_frames(b, pcm.reshape(-1, 1), 44100)
    assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.timeout(300)
def test_mix_plan_under_asan_ubsan(tmp_path):
    """csrc/mix_plan.cpp makes no HIP call: built with g++ and the sanitizers, then fed random mixes (items across and past
    track_len, zero-length rows, 10 000 items on one track) and invalid arguments by tests/sanitize_mix_driver.cpp, which
    checks the invariants of every plan."""
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-ffp-contract=off", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "mix_plan.cpp"), os.path.join(ROOT, "tests", "sanitize_mix_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_mix_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize mix driver: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_dialogue_example_builds_and_fails_loudly_without_a_device(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    if G.device_count() == 0:   # no CPU fallback: the example must fail loudly, not write silence
        r = subprocess.run([exe, "-o", os.devnull, "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
