"""The filter-stream kernels inside libgrail_hip.so, read without a GPU: both instantiations of fir_stream_kernel and the
advance kernel are there, compiled for gfx950 only (the fixture refuses any other code object), with no private segment and
no spills (the eight accumulators and the window of fifteen samples stay in registers, as in fir_kernel, whose loop they
share: DESIGN.md §4.15), wavefront size 64, and the stretch of fir_kernel in LDS."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)


def test_fir_stream_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    stream = {name: meta for name, meta in kernels.items() if re.search(r"fir_stream_(advance_)?kernel", name)}
    vec = sorted(m.group(1) for m in (re.search(r"fir_stream_kernelILb([01])E", name) for name in stream) if m)
    assert vec == ["0", "1"], sorted(stream)
    assert sum("fir_stream_advance_kernel" in name for name in stream) == 1 and len(stream) == 3, sorted(stream)
    for name, meta in stream.items():
        assert meta["private_segment_fixed_size"] == 0, (name, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] == 256, (name, meta)
        if "advance" in name:
            assert meta["group_segment_fixed_size"] == 0, (name, meta)
        else:
            # the stretch in LDS: 8 rows of 772 words and the four counts; room for four waves a SIMD
            assert 8 * 772 * 4 <= meta["group_segment_fixed_size"] <= 8 * 772 * 4 + 64, (name, meta)
            assert meta["vgpr_count"] <= 128 and meta["agpr_count"] == 0, (name, meta)


def test_the_one_shot_kernels_kept_their_figures(kernels):
    """fir_kernel shares its tap loop with the stream kernel through one inline function: its registers and LDS are what
    they were before the loop moved there (66 VGPRs, 24 720 bytes: DESIGN.md §4.14)"""
    one_shot = {name: meta for name, meta in kernels.items() if re.search(r"fir_kernelILb[01]E", name)}
    assert len(one_shot) == 2, sorted(one_shot)
    for name, meta in one_shot.items():
        assert meta["vgpr_count"] == 66 and meta["group_segment_fixed_size"] == 24720, (name, meta)
