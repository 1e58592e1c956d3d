"""grail_track_dyn_async (include/grail_hip.h, "levels, continued: dynamics, a workgroup a row") without a GPU: the header
declares the call under its own heading and says which call is for what, the binding and both Rust crates name it, its
arguments are grail_dyn_async's, every refusal of dyn_call_error comes back with the words grail_dyn_async gives for the same
arguments under the new call's name, before the device is looked for, and grail_dialogue knows --compress-tracks."""
import ctypes as C
import os
import re
import subprocess

import grail_hip as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "grail_track_dyn_async"


def test_header_binding_and_crates_declare_the_call(built):
    hdr = open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    heading = hdr.index("levels, continued: dynamics, a workgroup a row")
    streams = hdr.index("levels, continued: dynamics of streams")
    assert hdr.index("/* ---- levels, continued: dynamics ----") < heading < streams     # directly after the dynamics section
    section = hdr[heading:streams]
    assert "WHICH CALL FOR WHAT" in section and "THE BITS are those of ROW above, whatever the number of rows" in section
    assert "there is no form parallel in time" not in re.sub(r"\s*\n \*\s*", " ", hdr)
    code = re.sub(r"/\*.*?\*/", "", section, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, code)
    # the parameters are grail_dyn_async's, in its order
    whole = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    params = {n: re.sub(r"\s+", " ", re.search(r"\bint %s\s*\((.*?)\)\s*;" % n, whole, flags=re.S).group(1)) for n in (NAME, "grail_dyn_async")}
    assert params[NAME] == params["grail_dyn_async"]
    lib = G.load()
    assert NAME in G.EXPORTS and lib.grail_track_dyn_async.argtypes == lib.grail_dyn_async.argtypes
    assert lib.grail_track_dyn_async.argtypes is not None and len(lib.grail_track_dyn_async.argtypes) == 17
    sys_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip-sys", "src", "lib.rs")).read()
    safe_rs = open(os.path.join(ROOT, "grail-rs_amd", "rust", "grail-hip", "src", "lib.rs")).read()
    assert re.search(r"pub fn %s\s*\(" % NAME, sys_rs) and ("sys::" + NAME) in safe_rs and "pub fn track_dynamics" in safe_rs
    for method in ("track_dyn_async", "track_dyn"):
        assert callable(getattr(G.Context, method)), method
    # no define of the dynamics block is new, and the tile is a power of two the kernel's tests can read
    plan = open(os.path.join(ROOT, "grail-rs_amd", "csrc", "dyn_plan.h")).read()
    tile = int(re.search(r"constexpr uint32_t TRACK_TILE = (\d+);", plan).group(1))
    assert 256 <= tile <= 4096 and tile & (tile - 1) == 0


def test_every_refusal_is_grail_dyn_asyncs_under_the_calls_own_name(built):
    lib = G.load()
    a, b, k, ln, fake = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000      # addresses nobody looks behind
    # (ctx, set, rows, row_stride, len, n_rows, curve, key, key_stride, key_len, n_keys, key_row, out, out_stride, 3 results)
    cases = [
        ((None, None, a, 64, ln, 1, None, None, 0, None, 0, None, b, 64, None, None, None), b"set is NULL"),
        ((None, None, a, 64, ln, 0, None, None, 0, None, 0, None, b, 64, None, None, None), b"set is NULL"),
        ((None, fake, a, 64, None, 1, None, None, 0, None, 0, None, b, 64, None, None, None), b"NULL buffer"),
        ((None, fake, None, 64, ln, 1, None, None, 0, None, 0, None, b, 64, None, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 1, None, None, 0, None, 0, None, None, 64, None, None, None), b"NULL buffer"),
        ((None, fake, a, 64, ln, 2, None, None, 0, None, 0, None, a + 4 * 64, 64, None, None, None), b"overlaps rows_dev"),
        ((None, fake, a, 64, ln, 1, None, None, 0, None, 0, None, a, 64, None, None, None), b"overlaps rows_dev"),
        ((None, fake, a, 2 ** 32, ln, 1, None, None, 0, None, 0, None, 2 ** 50, 2 ** 32, None, None, None), b"2^32 output samples"),
        ((None, fake, a, 2 ** 59, ln, 4, None, None, 0, None, 0, None, 2 ** 62, 64, None, None, None), b"2^60 samples"),
        ((None, fake, a, 64, ln, 2, None, k, 64, None, 0, None, b, 64, None, None, None), b"n_keys = 0"),
        ((None, fake, a, 64, ln, 2, None, k, 64, None, 1, None, b, 64, None, None, None), b"n_keys < n_rows"),
        ((None, fake, a, 64, ln, 2, None, k, 2 ** 59, None, 4, None, b, 64, None, None, None), b"2^60 samples"),
        ((None, fake, a, 64, ln, 2, None, b + 4 * 127, 64, None, 2, None, b, 64, None, None, None), b"overlaps key_dev"),
        ((None, fake, a, 64, ln, 2, None, b - 4 * 64 + 4, 64, None, 1, ln, b, 64, None, None, None), b"overlaps key_dev"),
    ]
    for args, word in cases:
        assert lib.grail_dyn_async(*args) == G.ERR_INVALID_ARG, args
        serial = lib.grail_last_error()
        assert lib.grail_track_dyn_async(*args) == G.ERR_INVALID_ARG, args
        mine = lib.grail_last_error()
        assert word in mine and NAME.encode() in mine, (args, mine)
        assert mine == serial.replace(b"grail_dyn_async", NAME.encode()), (serial, mine)      # the same words, the call's own name
    # a workgroup a row: a grid of 2^31 workgroups does not fit (the one refusal of its own, after dyn_call_error's)
    big = (None, fake, a, 0, ln, 2 ** 31, None, None, 0, None, 0, None, None, 0, None, None, None)
    # (grail_dyn_async passes every check of these arguments: it ends at the device, or at the context that is NULL)
    assert lib.grail_dyn_async(*big) != G.OK and b"workgroups" not in lib.grail_last_error()
    assert lib.grail_track_dyn_async(*big) == G.ERR_INVALID_ARG and b"more than 2^31 workgroups" in lib.grail_last_error()
    if G.device_count() == 0:        # no context can exist: the valid calls say why, they do not compute on the CPU
        assert lib.grail_track_dyn_async(None, fake, a, 64, ln, 2, None, k, 64, None, 1, ln, b, 64, None, None, None) == G.ERR_NO_DEVICE
        assert b"no usable HIP device" in lib.grail_last_error() and NAME.encode() in lib.grail_last_error()
        assert lib.grail_track_dyn_async(None, fake, None, 0, None, 0, None, None, 0, None, 0, None, None, 0, None, None, None) == G.ERR_NO_DEVICE
        assert lib.grail_track_dyn_async(None, fake, a, 0, ln, 2 ** 31 - 1, None, None, 0, None, 0, None, None, 0, None, None, None) == G.ERR_NO_DEVICE
    else:                           # a set of another context is looked up, not looked into
        one, two = G.Context(0), G.Context(0)
        try:
            flat = (G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, -24.0, 4.0, 6.0, 0.0, 0.0), (0.5, 0.9), G.DYN_PEAK)
            theirs = one.dyn_create([flat])
            args = (theirs, a, 64, ln, 1, None, None, 0, None, 0, None, b, 64, None, None, None)
            assert lib.grail_track_dyn_async(two.handle, *args) == G.ERR_INVALID_ARG
            assert b"grail_track_dyn_async: not a curve set of this context" in lib.grail_last_error()
            assert lib.grail_track_dyn_async(two.handle, C.c_void_p(fake), *args[1:]) == G.ERR_INVALID_ARG
            # (its own context takes it: nothing to do for no rows)
            assert lib.grail_track_dyn_async(one.handle, theirs, a, 64, ln, 0, None, None, 0, None, 0, None, b, 64, None, None, None) == G.OK
            one.dyn_free(theirs)
        finally:
            one.close()
            two.close()


def test_dialogue_example_knows_compress_tracks(built):
    exe = os.path.join(ROOT, "grail-rs_amd", "lib", "grail_dialogue")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "[--makeup DB]] [--compress-tracks] [--rate R]" in r.stderr
    r = subprocess.run([exe, "--compress-tracks", "a", "e"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr and "[--compress-tracks]" in r.stderr
    if G.device_count() == 0:
        r = subprocess.run([exe, "-o", os.devnull, "--compress", "-24:3:6:5:120", "--compress-tracks", "a", "e"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
