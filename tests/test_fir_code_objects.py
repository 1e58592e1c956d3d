"""The FIR kernels inside libgrail_hip.so, read without a GPU: both instantiations of fir_kernel and the totals kernel are
there, compiled for gfx950 only (the fixture refuses any other code object), with no private segment and no spills (the
eight accumulators and the window of fifteen samples stay in registers: DESIGN.md §4.14), wavefront size 64."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)


def test_fir_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    fir = {name: meta for name, meta in kernels.items() if re.search(r"fir_(totals_)?kernel", name)}
    vec = sorted(m.group(1) for m in (re.search(r"fir_kernelILb([01])E", name) for name in fir) if m)
    assert vec == ["0", "1"], sorted(fir)
    assert sum("fir_totals_kernel" in name for name in fir) == 1 and len(fir) == 3, sorted(fir)
    for name, meta in fir.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] == 256, (name, meta)
        if "totals" not in name:
            # the stretch in LDS: 8 rows of 772 words and the four counts; room for four waves a SIMD
            assert 8 * 772 * 4 <= meta["group_segment_fixed_size"] <= 8 * 772 * 4 + 64, (name, meta)
            assert meta["vgpr_count"] <= 128 and meta["agpr_count"] == 0, (name, meta)
