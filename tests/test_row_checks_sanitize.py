"""The row-pair check that every call which writes rows makes (csrc/row_checks.h: header-only, no HIP type) under
AddressSanitizer and UBSan: built with plain g++ into a stand-alone driver with its own main
(tests/sanitize_row_checks_driver.cpp), as tests/test_fir_stream_sanitize.py does for the stream checks that call it.
Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_row_checks_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g", "-O1", "-std=c++17",
           "-Wall", "-Wextra", "-Werror"]
    exe = str(tmp_path / "sanitize_row_checks_driver")
    subprocess.check_call(["g++", *san, os.path.join(ROOT, "tests", "sanitize_row_checks_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=250)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitize row checks driver: ok" in r.stdout
