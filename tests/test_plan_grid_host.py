"""The launch planner over a grid of contexts and batches built directly, recorded: tests/plan_grid_driver.cpp sweeps device
sizes, arithmetics, voice tables, aligned and ragged rows, phoneme batches and caller-built elems, every option of the
planner off its default and six block sizes, and prints every family choose_family gives (also exact-only and with the lanes
pinned), its prices, the packed order and the batch's plan.  tests/golden/plan_grid.txt holds, per group of 12 cells, the
sha256 of what the planner answered while it was one file (launch_plan.cpp, 1 024 lines); a change of the host code that is
not meant to move a plan must repeat it byte for byte.  The driver also checks its own coverage (every option moves a line,
every family kind occurs) and fails if the grid no longer reaches it.  No GPU needed.  Run as a script, the module writes
the golden file (to the path given, else to stdout)."""
import hashlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_grid.txt")

# the units that make up the planner (the only thing that differs between recording and replay), and what they need
PLANNER_UNITS = ("launch_plan.cpp", "family_choice.cpp", "family_cost.cpp", "dispatch_model.cpp")
OTHER_UNITS = ("voice_analysis.cpp", "voice_host.cpp")
FLAGS = ["-O1", "-ffp-contract=off", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]


def _build(out_dir, extra=()):
    csrc = os.path.join(ROOT, "grail-rs_amd", "csrc")
    exe = os.path.join(str(out_dir), "plan_grid_driver")
    subprocess.check_call(["g++", *FLAGS, *extra, os.path.join(ROOT, "tests", "plan_grid_driver.cpp"),
                           *(os.path.join(csrc, u) for u in PLANNER_UNITS + OTHER_UNITS), "-o", exe, "-lm"])
    return exe


def _groups(text):
    """[(header line, the group's text)] of the driver's output"""
    groups = []
    for line in text.splitlines(keepends=True):
        if line.startswith("== "):
            groups.append((line[3:].rstrip("\n"), ""))
        else:
            groups[-1] = (groups[-1][0], groups[-1][1] + line)
    return groups


def _digest(groups):
    return "".join(f"{key} sha256={hashlib.sha256(body.encode()).hexdigest()}\n" for key, body in groups)


def test_every_cell_of_the_grid_repeats_the_recorded_planner(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=250)
    assert r.returncode == 0, r.stderr[-4000:]          # (non-zero: a coverage condition of the driver failed)
    groups = _groups(r.stdout)
    recorded = open(GOLDEN).read()
    assert len(recorded) < 64 * 1024
    want = recorded.splitlines()
    assert len(groups) == len(want)
    for (key, body), line, mine in zip(groups, want, _digest(groups).splitlines()):
        if mine != line:
            path = tmp_path / "group_got.txt"
            path.write_text(body)
            pytest.fail(f"group [{key}] differs from the recorded planner (recorded: {line}); its text is in {path}")
    assert _digest(groups) == recorded


@pytest.mark.timeout(300)
def test_the_grid_under_asan_ubsan(tmp_path):
    """the same driver and grid with AddressSanitizer + UBSan, as a stand-alone program: it only has to come back clean"""
    exe = _build(tmp_path, ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined", "-g"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=280)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        digest = _digest(_groups(subprocess.run([_build(tmp)], capture_output=True, text=True, check=True).stdout))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(digest)
    else:
        sys.stdout.write(digest)
