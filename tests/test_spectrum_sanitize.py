"""The pure-host side of short-time spectra (csrc/spectrum_plan.cpp: grail_spectrum_twiddles, grail_spectrum_frames,
grail_spectrum_window, grail_mel_design, a set's checks and image, the checks and the grid of grail_spectrum_async) under
AddressSanitizer and UBSan: built with g++ beside a stand-alone driver with its own main (tests/sanitize_spectrum_driver.cpp),
which runs the designers at p = 6 and p = 12 into arrays of exactly the size they may write, puts bands at both edges of
0 .. N/2, and goes through every refusal.  The unit is built without -ffp-contract=off on purpose: it switches contraction off
itself.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_spectrum_plan_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "spectrum_plan.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_spectrum_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_spectrum_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize spectrum driver: ok" in r.stdout
