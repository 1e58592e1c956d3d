"""The resample-stream kernels inside libgrail_hip.so, read without a GPU: the ten instantiations of resample_stream_kernel
and the advance kernel are there, compiled for gfx950 only (the fixture refuses any other code object), with no private
segment and no spills, wavefront size 64; and resample_kernel has the registers and the LDS it had before the stream kernel
came into its file (the stream kernel folds with a copy of its loop: sharing one inline function kept these figures and
still cost the one-shot call 0.5 % at full size).  Metadata only."""
import re

from test_code_objects import kernels  # noqa: F401  (a fixture)

# <STAGED, VEC, TAB>: TAB 0 = the table where it lies, 1 = one phase (wave-uniform), 2 = the table in LDS (staged only)
INSTANTIATIONS = sorted((s, v, t) for s in (0, 1) for v in (0, 1) for t in ((0, 1, 2) if s else (0, 1)))
# resample_kernel<STAGED, VEC, TAB>'s VGPRs in the commit before the stream kernels (VEC does not change them)
ONE_SHOT_VGPRS = {(0, 0): 51, (0, 1): 40, (1, 0): 44, (1, 1): 54, (1, 2): 62}
ONE_SHOT_LDS = 16       # the four counts; the stretch is dynamic LDS, sized by the launch


def instantiations(kernels, name):
    out = {}
    for symbol, meta in kernels.items():
        m = re.search(name + r"ILb([01])ELb([01])ELi([012])EEE", symbol)
        if m:
            out[tuple(int(g) for g in m.groups())] = meta
    return out


def test_resample_stream_kernels_are_in_the_library_without_scratch_or_spills(kernels):
    stream = instantiations(kernels, r"\d+resample_stream_kernel")
    assert sorted(stream) == INSTANTIATIONS, sorted(stream)
    advance = [meta for symbol, meta in kernels.items() if "resample_stream_advance_kernel" in symbol]
    assert len(advance) == 1
    for what, meta in list(stream.items()) + [("advance", advance[0])]:
        assert meta["private_segment_fixed_size"] == 0, (what, meta)
        assert meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (what, meta)
        assert meta["wavefront_size"] == 64 and meta["max_flat_workgroup_size"] == 256, (what, meta)
        assert meta["agpr_count"] == 0, (what, meta)
    assert advance[0]["group_segment_fixed_size"] == 0
    for what, meta in stream.items():
        # room for four workgroups a compute unit, as the one-shot kernel has
        assert meta["group_segment_fixed_size"] == ONE_SHOT_LDS and meta["vgpr_count"] <= 128, (what, meta)


def test_the_one_shot_kernels_kept_their_figures(kernels):
    one_shot = instantiations(kernels, r"\d+resample_kernel")
    assert sorted(one_shot) == INSTANTIATIONS, sorted(one_shot)
    for (staged, vec, tab), meta in one_shot.items():
        assert meta["vgpr_count"] == ONE_SHOT_VGPRS[(staged, tab)], ((staged, vec, tab), meta)
        assert meta["group_segment_fixed_size"] == ONE_SHOT_LDS, ((staged, vec, tab), meta)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0, ((staged, vec, tab), meta)
