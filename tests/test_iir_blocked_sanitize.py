"""The pure-host side of recursive filtering parallel in time (csrc/iir_plan.cpp: grail_biquad_block_matrix, a set's matrix image,
the grid and the scratch size of grail_biquad_blocked_async) under AddressSanitizer and UBSan: built with g++ beside a stand-alone
driver with its own main (tests/sanitize_iir_blocked_driver.cpp), which fills matrices of exactly [2 S][2 S] doubles for
S = 1 .. 8, goes through every refusal, and walks the sizes at row_stride 0, 1, 1024 and 2^32 - 1 with a tail of 0 and of
2^32 - 1.  The matrix is built without -ffp-contract=off on purpose: the unit switches contraction off itself."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_iir_block_plan_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "iir_plan.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_iir_blocked_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_iir_blocked_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize iir blocked driver: ok" in r.stdout
