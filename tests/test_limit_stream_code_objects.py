"""The limit-stream kernels inside libgrail_hip.so, read without a GPU: both instantiations of limit_stream_kernel and the
advance kernel are there, compiled for gfx950 only (the fixture refuses any other code object), with no private segment and
no spills, wavefront size 64, no AGPRs, their LDS small enough for three workgroups a compute unit; and limit_frames_kernel
has the registers and the LDS it had before the stream kernels came into its file (the stream kernel detects with a copy of
limit_detect: limit_frames_kernel is textually unchanged).  Metadata only."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)

# limit_frames_kernel<VEC>'s VGPRs and LDS in the commit before the stream kernels ("Synthesis kernels: a ledger pins every
# instantiation by name to a cell"), read from that commit's limiter_kernels.hip built with the Makefile's flags and
# -Rpass-analysis=kernel-resource-usage: 56 and 54 VGPRs, 49 568 bytes (two arrays of 6 156 cells and four chunk records)
ONE_SHOT_VGPRS = {0: 56, 1: 54}
ONE_SHOT_LDS = 49568
LDS_PER_CU = 160 * 1024


def instantiations(kernels, name):
    out = {}
    for symbol, meta in kernels.items():
        m = re.search(name + r"ILb([01])EEE", symbol)
        if m:
            out[int(m.group(1))] = meta
    return out


def test_limit_stream_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    stream = instantiations(kernels, r"\d+limit_stream_kernel")
    assert sorted(stream) == [0, 1], sorted(stream)
    advance = [meta for symbol, meta in kernels.items() if "limit_stream_advance_kernel" in symbol]
    assert len(advance) == 1
    for what, meta in list(stream.items()) + [("advance", advance[0])]:
        assert meta["private_segment_fixed_size"] == 0, (what, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (what, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] <= 256, (what, meta)
        assert meta["agpr_count"] == 0, (what, meta)
    assert advance[0]["group_segment_fixed_size"] == 0                      # it needs no LDS
    for what, meta in stream.items():
        # the LDS plan of limit_frames_kernel: three workgroups a compute unit, and registers for them (12 waves: 3 a SIMD)
        assert meta["group_segment_fixed_size"] == ONE_SHOT_LDS and 3 * meta["group_segment_fixed_size"] <= LDS_PER_CU, (what, meta)
        assert meta["vgpr_count"] <= 128, (what, meta)


def test_the_one_shot_kernels_kept_their_figures(kernels):
    one_shot = instantiations(kernels, r"\d+limit_frames_kernel")
    assert sorted(one_shot) == [0, 1], sorted(one_shot)
    for vec, meta in one_shot.items():
        assert meta["vgpr_count"] == ONE_SHOT_VGPRS[vec], (vec, meta)
        assert meta["group_segment_fixed_size"] == ONE_SHOT_LDS, (vec, meta)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["agpr_count"] == 0, (vec, meta)
