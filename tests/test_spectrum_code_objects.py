"""The spectrum kernels inside libgrail_hip.so, read without a GPU: exactly the instantiations spectrum_kernel<P, VEC> for P =
6 .. 12 and both load widths (14) and spectrum_totals_kernel are there and no other kernel carries the name, compiled for
gfx950 only (the fixture refuses any other code object), wavefront size 64, with no private segment and no spills, the 256
lanes a workgroup the launcher gives them, and the LDS of DESIGN.md §4.25: N complex doubles a frame, four frames side by side
up to N = 256 and one from N = 512 on, N/2 twiddle pairs beside them, four words for the count: 98 320 bytes at N = 4096."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)


def lds_bytes(p):
    n = 1 << p
    side = 4 if p <= 8 else 1
    return side * n * 16 + (n // 2) * 16 + 4 * 4


def test_spectrum_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    mine = {name: meta for name, meta in kernels.items() if re.search(r"spectrum_", name)}
    frames = {name: meta for name, meta in mine.items() if "spectrum_kernel" in name}
    found = sorted(tuple(int(x) for x in m.groups()) for m in
                   (re.search(r"spectrum_kernelILj(\d+)ELb([01])EE", name) for name in frames) if m)
    assert found == sorted((p, vec) for p in range(6, 13) for vec in (0, 1)), sorted(mine)
    totals = [name for name in mine if "spectrum_totals_kernel" in name]
    assert len(frames) == len(found) == 14 and len(totals) == 1 and len(mine) == 15, sorted(mine)
    for name, meta in mine.items():
        for other in ("iir_", "fir_kernel", "fir_stream_", "meter_stream_", "biquad_block_", "dyn_", "track_"):
            assert other not in name, name             # (the neighbouring code-object tests count their kernels by these)
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] == 256, (name, meta)
        print(name, meta["vgpr_count"], meta["sgpr_count"], meta["group_segment_fixed_size"])
    for name, meta in frames.items():
        p = int(re.search(r"spectrum_kernelILj(\d+)E", name).group(1))
        assert meta["group_segment_fixed_size"] == lds_bytes(p), (name, meta)     # (to the byte: the three arrays need no padding)
        # two workgroups a CU at the least: 128 registers a lane and 80 KB of the 160 would do, but for N = 4096
        assert meta["vgpr_count"] <= 128, (name, meta)
    assert lds_bytes(12) == 98320
    assert kernels[totals[0]]["group_segment_fixed_size"] == 0
