"""The pure-host side of meter streams (csrc/meter_plan.cpp: the hop of a rate and grail_meter_stream_hops, the stride rule of a
call's hop sums, the checks of open and next, the chunk count) under AddressSanitizer and UBSan: built with g++ beside a
stand-alone driver with its own main (tests/sanitize_meter_stream_driver.cpp), as tests/test_limit_stream_sanitize.py does for
limit streams.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_meter_stream_plan_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1",
           "-ffp-contract=off", "-std=c++17"]
    objs = []
    for name in (os.path.join(ROOT, "grail-rs_amd", "csrc", "meter_plan.cpp"),
                 os.path.join(ROOT, "tests", "sanitize_meter_stream_driver.cpp")):
        o = str(tmp_path / (os.path.basename(name) + ".o"))
        subprocess.check_call(["g++", *san, "-c", name, "-o", o])
        objs.append(o)
    exe = str(tmp_path / "sanitize_meter_stream_driver")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", *objs, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize meter stream driver: ok" in r.stdout
