"""The IIR kernel inside libgrail_hip.so, read without a GPU: every instantiation of iir_kernel<section bound, VEC, STREAM> is
there (4 x 2 x 2) and no other kernel carries the name, compiled for gfx950 only (the fixture refuses any other code object),
wavefront size 64, with no private segment and no spills (the lane's 5 S coefficients and 2 S states are statically indexed
registers: DESIGN.md §4.19), and within the registers and the LDS that the occupancy stated there needs: two waves a SIMD
up to a section bound of four (eight one-wave workgroups a compute unit: at most 256 registers a lane), one wave a SIMD at a
bound of eight (at most 512), and 160 KB / 8 of LDS a workgroup either way."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)

BOUNDS = (1, 2, 4, 8)
WAVES_PER_SIMD = {1: 2, 2: 2, 4: 2, 8: 1}             # DESIGN.md §4.19, by section bound
LDS = 160 * 1024 // (4 * 2)


def test_iir_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    iir = {name: meta for name, meta in kernels.items() if re.search(r"iir_", name)}
    found = sorted(tuple(int(x) for x in m.groups()) for m in
                   (re.search(r"iir_kernelILj(\d+)ELb([01])ELb([01])EE", name) for name in iir) if m)
    assert found == sorted((sb, vec, stream) for sb in BOUNDS for vec in (0, 1) for stream in (0, 1)), sorted(iir)
    assert len(iir) == len(found) == 16, sorted(iir)
    for name, meta in iir.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] == 64, (name, meta)
        # the tile of 64 rows x 65 words and the rows' 64 output lengths
        assert 64 * 65 * 4 + 64 * 4 <= meta["group_segment_fixed_size"] <= LDS, (name, meta)
        bound = int(re.search(r"iir_kernelILj(\d+)E", name).group(1))
        # (the metadata's vgpr_count is the unified total: arch VGPRs + AGPRs)
        assert meta["vgpr_count"] <= 512 // WAVES_PER_SIMD[bound], (name, meta)
        print(name, meta["vgpr_count"], meta["sgpr_count"], meta["group_segment_fixed_size"])
