"""The constants that the path-coverage cases of the GPU suite mirror (tests/KERNEL_PATHS.md), held to the lines of csrc
that define them: a change of a block size, a threshold or a grid cap fails here instead of quietly moving a kernel's
variants and tails away from the shapes that were chosen to reach them.  Constants only, read from the sources' text; and,
from the same arithmetic the GPU cases assert, which variants and tails their shapes reach."""
import os
import re

import grail_hip as G
import test_fir_gpu as fir
import test_levels_gpu as levels
import test_limiter_gpu as limiter
import test_mix_gpu as mix
import test_resample_gpu as resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grail-rs_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, name):
    """the value of `constexpr <type> NAME = <integers, + - * / << and names defined the same way>;` in text"""
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    expr = re.sub(r"(\d+)[uU]?[lL]{0,2}\b", r"\1", m.group(1))
    expr = re.sub(r"[A-Z][A-Z0-9_]+", lambda n: str(constant(text, n.group(0))), expr)
    assert re.fullmatch(r"[\d\s+\-*/()<>]+", expr), (name, expr)
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


def test_the_chunk_sizes_are_the_sources():
    kernels, header = source("kernels.h"), open(os.path.join(ROOT, "include", "grail_hip.h")).read()
    for name, mirrored in (("FIR_CHUNK", G.FIR_CHUNK), ("RESAMPLE_CHUNK", G.RESAMPLE_CHUNK), ("LIMIT_CHUNK", G.LIMIT_CHUNK)):
        assert constant(kernels, name) == mirrored, name
        assert int(re.search(r"#define GRAIL_" + name + r"\s+(\d+)", header).group(1)) == mirrored, name
    assert (fir.CHUNK, resample.CHUNK, limiter.T) == (G.FIR_CHUNK, G.RESAMPLE_CHUNK, G.LIMIT_CHUNK)


def test_the_firs_block_of_taps():
    text = source("fir_kernels.hip") + source("kernels.h")
    assert constant(text, "FIR_OWN") == fir.BLOCK == 8
    assert re.search(r"const uint32_t blocks = Kp >> 3;", text)                         # blocks of 2^3 taps,
    assert re.search(r"for \(; k \+ 2u <= blocks; k \+= 2u\)", text)                    # taken in pairs,
    assert re.search(r"if \(k < blocks\) fir_block\(", text)                            # and the odd one after them
    assert [fir.blocks(K) for K in (16, 17, 24, 25, 32, 33, 40, 41)] == [2, 3, 3, 4, 4, 5, 5, 6]
    odd = [K for K in fir.TAPS if fir.blocks(K) % 2 == 1 and fir.blocks(K) >= 3]
    assert odd == [17, 24, 33, 40]


def test_the_resamplers_lds_limit_and_the_variants_it_decides():
    text = source("resample_kernels.hip") + source("kernels.h")
    assert constant(text, "RS_LDS_MAX") == resample.LDS_MAX == 65472
    assert constant(text, "RS_STAGE_SLACK") == resample.STAGE_SLACK == 8
    assert constant(text, "RS_THREADS") == 256
    assert re.search(r"\(uint64_t\)\(U - 1u\) \+ \(uint64_t\)\(RESAMPLE_CHUNK - 1u\) \* D\) / U \+ P \+ RS_STAGE_SLACK", text)
    assert re.search(r"table_bytes = \(uint64_t\)U \* \(P \+ 1u\) \* 4u", text)
    resample.test_the_pairs_and_layouts_reach_every_variant_of_the_kernel()
    # a stretch that just fits and one that just does not: U = 1, P + 1023 D + 8 + 1024 words against 16 368
    assert resample.variant(1, 14, 1014, True)[0] == "staged" and resample.variant(1, 14, 1015, True)[0] == "unstaged"


def test_the_limiters_32_bit_passes():
    text = source("limiter_kernels.hip") + source("kernels.h")
    assert constant(text, "LIMIT_SUM_LOG2") == limiter.SUM_LOG2 == 7
    assert constant(text, "LIMIT_Q") == 1 << 24
    assert (1 << limiter.SUM_LOG2) * (1 << 24) < 1 << 32                                 # what the passes are sized for
    assert limiter.ELLS == list(range(11)) and constant(text, "LIMIT_LMAX") == 1 << max(limiter.ELLS)
    assert sorted({(1 << ell) >> min(ell, limiter.SUM_LOG2) for ell in limiter.ELLS}) == [1, 2, 4, 8]      # pieces at the apply


def test_the_frames_grid_cap():
    text = source("mix_kernels.hip")
    m = re.search(r"pcm16_frames_kernel, dim3\(\(uint32_t\)\(groups < (\d+)u \? groups : (\d+)u\)\), dim3\((\d+)\)", text)
    assert m and int(m.group(1)) == int(m.group(2)) == mix.FRAMES_GRID_CAP == 65536 and int(m.group(3)) == 256
    assert re.search(r"e \+= \(uint64_t\)gridDim\.x \* 256u", text)


def test_the_level_frames_steps():
    text = source("level_kernels.hip")
    assert constant(text, "LEVEL_CHUNKS") == levels.LEVEL_CHUNKS == 8
    assert re.search(r"if \(c1 - c > 4u\) level_step<VEC, 8>.*\n\s*else if \(c1 - c > 2u\) level_step<VEC, 4>.*\n\s*"
                     r"else if \(c1 > c\) level_step<VEC, 2>", text)
    reached = set().union(*(levels.level_steps(n, F) for n in levels.LENGTHS for F in levels.FRAMES))
    assert reached == {"full", "tail2", "tail4"}                                         # (KERNEL_PATHS.md: who reaches tail8)
    assert "tail8" in levels.level_steps(20000, G.LEVEL_FRAME)                           # test_scratch_reuse_gpu.py's shape B


def test_every_line_of_the_census_names_a_test_that_exists():
    """tests/KERNEL_PATHS.md: every row of its tables names, in its last column, test ids `file.py::name` that exist"""
    with open(os.path.join(ROOT, "tests", "KERNEL_PATHS.md")) as f:
        rows = [line for line in f if line.startswith("|") and not re.match(r"\|\s*(-+|kernel)\s*\|", line)]
    assert len(rows) > 60
    defined = {}
    for line in rows:
        ids = re.findall(r"`(test_\w+\.py)::(test_\w+)", line.rstrip().rstrip("|").split("|")[-1])
        assert ids, "a line without a test id: " + line
        for name, test in ids:
            if name not in defined:
                with open(os.path.join(ROOT, "tests", name)) as f:
                    defined[name] = set(re.findall(r"^def (test_\w+)\(", f.read(), re.M))
            assert test in defined[name], (name, test)
