"""The workgroup-a-row dynamics kernel inside libgrail_hip.so, read without a GPU: every instantiation of
track_env_kernel<VEC, KEYED> is there (2 x 2) and no other kernel carries track_env_, none of their names holds a substring a
neighbouring code-object test counts its kernels by, compiled for gfx950 only (the fixture refuses any other code object),
wavefront size 64, no private segment and no spills, a workgroup of the TRACK_THREADS lanes the launcher launches (one chain
wave and TRACK_TILE / 4 workers), the LDS of DESIGN.md §4.24 (two tiles of TRACK_TILE doubles and, for the row's end, a double
and two words a worker: no curve is staged), and at most the 64 registers a lane §4.24 claims (eight waves a SIMD, so six
workgroups of five waves a CU)."""
import os
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = open(os.path.join(ROOT, "grail-rs_amd", "csrc", "dyn_plan.h")).read()
TILE = int(re.search(r"constexpr uint32_t TRACK_TILE = (\d+);", PLAN).group(1))
WORKERS = TILE // 4
THREADS = 64 + WORKERS
LDS = 2 * TILE * 8 + WORKERS * (8 + 4 + 4)
SLACK = 64                                             # alignment


def test_the_plan_header_says_the_same():
    assert re.search(r"constexpr uint32_t TRACK_WORKERS = TRACK_TILE / 4;", PLAN)
    assert re.search(r"constexpr uint32_t TRACK_THREADS = 64 \+ TRACK_WORKERS;", PLAN)
    assert 256 <= TILE <= 4096 and TILE & (TILE - 1) == 0 and THREADS <= 1024
    src = open(os.path.join(ROOT, "grail-rs_amd", "csrc", "track_env_kernels.hip")).read()
    assert len(re.findall(r"dim3\(TRACK_THREADS\)", src)) == 2 and "__launch_bounds__(TRACK_THREADS)" in src
    assert "atomic" not in src.replace("No atomics", "")


def test_track_env_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    mine = {name: meta for name, meta in kernels.items() if "track_env_" in name}
    found = sorted(tuple(int(x) for x in m.groups()) for m in
                   (re.search(r"track_env_kernelILb([01])ELb([01])EE", name) for name in mine) if m)
    assert found == sorted((vec, keyed) for vec in (0, 1) for keyed in (0, 1)), sorted(mine)
    assert len(mine) == len(found) == 4, sorted(mine)
    for name, meta in mine.items():
        for other in ("dyn_", "iir_", "fir_kernel", "fir_stream_", "meter_stream_", "biquad_block"):
            assert other not in name, name             # (the neighbouring code-object tests count their kernels by these)
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] == THREADS, (name, meta)
        assert LDS <= meta["group_segment_fixed_size"] <= LDS + SLACK, (name, meta)
        # (the metadata's vgpr_count is the unified total: arch VGPRs + AGPRs)
        assert meta["vgpr_count"] <= 64, (name, meta)
        print(name, meta["vgpr_count"], meta["sgpr_count"], meta["group_segment_fixed_size"])
