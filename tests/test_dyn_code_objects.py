"""The dynamics kernel inside libgrail_hip.so, read without a GPU: every instantiation of dyn_kernel<VEC, KEYED, STREAM> is there
(2 x 2 x 2) and no other kernel carries the name, compiled for gfx950 only (the fixture refuses any other code object), wavefront
size 64, with no private segment and no spills, at most 256 registers a lane (arch VGPRs + AGPRs: two waves a SIMD), and the
LDS of DESIGN.md §4.23: one tile of 64 rows x 65 words and the rows' 64 output lengths unkeyed; a second tile and the rows' 64
key indices keyed; no curve is staged (the table is gathered from global memory), so nothing beyond a few bytes of padding."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)

TILE = 64 * 65 * 4
WORDS = 64 * 4
SLACK = 64                                             # alignment, and the one-word stand-ins of the unkeyed instantiations


def test_dyn_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    dyn = {name: meta for name, meta in kernels.items() if re.search(r"dyn_", name)}
    found = sorted(tuple(int(x) for x in m.groups()) for m in
                   (re.search(r"dyn_kernelILb([01])ELb([01])ELb([01])EE", name) for name in dyn) if m)
    assert found == sorted((vec, keyed, stream) for vec in (0, 1) for keyed in (0, 1) for stream in (0, 1)), sorted(dyn)
    assert len(dyn) == len(found) == 8, sorted(dyn)
    for name, meta in dyn.items():
        for other in ("iir_", "fir_kernel", "fir_stream_", "meter_stream_", "biquad_block_"):
            assert other not in name, name             # (the neighbouring code-object tests count their kernels by these)
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] == 64, (name, meta)
        keyed = int(re.search(r"dyn_kernelILb[01]ELb([01])E", name).group(1))
        lds = (TILE + WORDS) * (2 if keyed else 1)
        assert lds <= meta["group_segment_fixed_size"] <= lds + SLACK, (name, meta)
        # (the metadata's vgpr_count is the unified total: arch VGPRs + AGPRs)
        assert meta["vgpr_count"] <= 256, (name, meta)
        print(name, meta["vgpr_count"], meta["sgpr_count"], meta["group_segment_fixed_size"])
