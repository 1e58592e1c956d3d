"""The kernels of recursive filtering parallel in time inside libgrail_hip.so, read without a GPU: every instantiation of
biquad_block_kernel<section bound, VEC, OUT> (4 x 2 x 2), the four biquad_block_propagate_kernel<section bound> and the
totals kernel are there, compiled for gfx950 only (the fixture refuses any other code object), wavefront size 64, with no
private segment and no spills (coefficients, states and a row of the block matrix are statically indexed registers: DESIGN.md
section 4.22), within two waves a SIMD up to a section bound of four (at most 256 registers a lane) and one at eight (at most
512), and 160 KB / 8 of LDS a workgroup.  None of their names contains "iir_": tests/test_iir_code_objects.py counts the
sixteen kernels that do, and passes unchanged."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)

BOUNDS = (1, 2, 4, 8)
LDS = 160 * 1024 // (4 * 2)


def test_block_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    mine = {name: meta for name, meta in kernels.items() if "biquad_block" in name}
    block = sorted(tuple(int(x) for x in m.groups()) for m in
                   (re.search(r"biquad_block_kernelILj(\d+)ELb([01])ELb([01])EE", name) for name in mine) if m)
    assert block == sorted((sb, vec, out) for sb in BOUNDS for vec in (0, 1) for out in (0, 1)), sorted(mine)
    propagate = sorted(int(m.group(1)) for m in
                       (re.search(r"biquad_block_propagate_kernelILj(\d+)EE", name) for name in mine) if m)
    assert propagate == list(BOUNDS), sorted(mine)
    totals = [name for name in mine if "biquad_block_totals_kernel" in name]
    assert len(totals) == 1 and len(mine) == 16 + 4 + 1, sorted(mine)
    for name, meta in mine.items():
        assert "iir_" not in name, name
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["wavefront_size"] == 64, (name, meta)
        assert meta["group_segment_fixed_size"] <= LDS, (name, meta)
        m = re.search(r"_kernelILj(\d+)E", name)
        bound = int(m.group(1)) if m else 1
        # (the metadata's vgpr_count is the unified total: arch VGPRs + AGPRs)
        assert meta["vgpr_count"] <= (512 if bound == 8 else 256), (name, meta)
        if "biquad_block_kernel" in name:
            assert meta["max_flat_workgroup_size"] == 64 and meta["group_segment_fixed_size"] >= 64 * 65 * 4, (name, meta)
        if "propagate" in name:
            assert meta["max_flat_workgroup_size"] == 64 and meta["group_segment_fixed_size"] == 0, (name, meta)
        print(name, meta["vgpr_count"], meta["sgpr_count"], meta["group_segment_fixed_size"])
