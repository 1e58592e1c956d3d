"""The meter-stream kernels inside libgrail_hip.so, read without a GPU: both instantiations of the hops and the peak kernel and
exactly one advance and one read kernel are there, compiled for gfx950 only (the fixture refuses any other code object), with
no private segment and no spills, wavefront size 64, no AGPRs; the hops kernel has the one-shot kernel's LDS (the same tile);
and the one-shot kernels whose arithmetic the stream kernels share (loudness_hops_kernel, loudness_gate_kernel,
true_peak_frames_kernel) have the registers and the LDS they had before: their files are textually unchanged, the stream
kernels restate what they could not include.  Metadata only."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)

# VGPRs and LDS of the one-shot kernels in the commit before the meter streams ("Stream tests: rows fed past 2^32 samples,
# calls of over 64 chunks"), read from that commit's loudness_kernels.hip and true_peak_kernels.hip built with the Makefile's
# flags and -Rpass-analysis=kernel-resource-usage: loudness_hops_kernel<VEC> 136 VGPRs either way and 16 640 bytes (the tile of
# 64 rows at pitch 65), loudness_gate_kernel 32 and none, true_peak_frames_kernel<VEC> 106 (4-byte loads) and 92 (16-byte) and none
HOPS_VGPRS = {0: 136, 1: 136}
HOPS_LDS = 64 * 65 * 4
GATE_VGPRS = 32
FRAMES_VGPRS = {0: 106, 1: 92}


def instantiations(kernels, name):
    out = {}
    for symbol, meta in kernels.items():
        m = re.search(name + r"ILb([01])EEE", symbol)
        if m:
            assert int(m.group(1)) not in out, symbol
            out[int(m.group(1))] = meta
    return out


def the_one(kernels, name):
    found = [meta for symbol, meta in kernels.items() if re.search(r"\d+" + name + r"E", symbol)]
    assert len(found) == 1, (name, len(found))
    return found[0]


def test_meter_stream_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    hops = instantiations(kernels, r"\d+meter_stream_hops_kernel")
    peak = instantiations(kernels, r"\d+meter_stream_peak_kernel")
    assert sorted(hops) == [0, 1] and sorted(peak) == [0, 1], (sorted(hops), sorted(peak))
    advance, read = the_one(kernels, "meter_stream_advance_kernel"), the_one(kernels, "meter_stream_read_kernel")
    assert len([s for s in kernels if "meter_stream_" in s]) == 6
    every = [(("hops", v), m) for v, m in hops.items()] + [(("peak", v), m) for v, m in peak.items()] + [("advance", advance), ("read", read)]
    for what, meta in every:
        assert meta["private_segment_fixed_size"] == 0, (what, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (what, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] <= 256, (what, meta)
        assert meta["agpr_count"] == 0, (what, meta)
    for what, meta in hops.items():
        assert meta["group_segment_fixed_size"] == HOPS_LDS and meta["max_flat_workgroup_size"] == 64, (what, meta)
        # the one-shot kernel's three waves a SIMD (512 / 3 = 170 registers, in steps of 8)
        assert meta["vgpr_count"] <= 168, (what, meta)
    for what, meta in list(peak.items()) + [("advance", advance), ("read", read)]:
        assert meta["group_segment_fixed_size"] == 0, (what, meta)


def test_the_one_shot_kernels_kept_their_figures(kernels):
    hops = instantiations(kernels, r"\d+loudness_hops_kernel")
    frames = instantiations(kernels, r"\d+true_peak_frames_kernel")
    assert sorted(hops) == [0, 1] and sorted(frames) == [0, 1]
    for vec, meta in hops.items():
        assert meta["vgpr_count"] == HOPS_VGPRS[vec] and meta["group_segment_fixed_size"] == HOPS_LDS, (vec, meta)
    for vec, meta in frames.items():
        assert meta["vgpr_count"] == FRAMES_VGPRS[vec] and meta["group_segment_fixed_size"] == 0, (vec, meta)
    gate = the_one(kernels, "loudness_gate_kernel")
    assert gate["vgpr_count"] == GATE_VGPRS and gate["group_segment_fixed_size"] == 0, gate
    for meta in list(hops.values()) + list(frames.values()) + [gate]:
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["agpr_count"] == 0, meta
