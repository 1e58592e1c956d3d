"""The pure-host side of recursive filtering (csrc/iir_plan.cpp: the designer, the checks and the image of a filter set, the
length rule, the checks of the calls on IIR streams) under AddressSanitizer and UBSan: built with g++ beside a stand-alone
driver with its own main (tests/sanitize_iir_driver.cpp), which designs into heap arrays of exactly five doubles, builds set
images for S = 1, 7, 8 and F = 1, 64, and goes through every refused argument."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_iir_plan_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-ffp-contract=off", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "iir_plan.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_iir_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_iir_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize iir driver: ok" in r.stdout
