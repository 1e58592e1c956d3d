"""The pure-host side of dynamics (csrc/dyn_plan.cpp: grail_dyn_design, grail_dyn_ballistics, lev[k], the lookup's index
arithmetic, a set's checks and image, the checks of grail_dyn_async and of the stream calls) under AddressSanitizer and UBSan:
built with g++ beside a stand-alone driver with its own main (tests/sanitize_dyn_driver.cpp), which designs into exactly 641
doubles, walks the index arithmetic at e = 0, a denormal, 2^-32 and its neighbours, every lev[k] and its predecessor, 2^8 and
the largest double, and goes through every refusal.  The unit is built without -ffp-contract=off on purpose: it switches
contraction off itself."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_dyn_plan_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "dyn_plan.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_dyn_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_dyn_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize dyn driver: ok" in r.stdout
