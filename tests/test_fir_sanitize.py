"""The pure-host side of FIR filtering (csrc/fir_plan.cpp: length, design, the checks and the padded image of a filter set,
with the sinc and I0 it shares from csrc/resample_plan.cpp) under AddressSanitizer and UBSan: built with g++ beside a
stand-alone driver with its own main (tests/sanitize_fir_driver.cpp), which designs into heap arrays of exactly K floats,
builds set images for K = 1, 7, 8, 9 and 4096, and goes through every refused argument."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_fir_plan_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-ffp-contract=off", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "fir_plan.cpp"),
                 os.path.join(ROOT, "grail-rs_amd", "csrc", "resample_plan.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_fir_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_fir_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize fir driver: ok" in r.stdout
