"""The constants that the path-coverage cases of the GPU suite mirror (tests/KERNEL_PATHS.md), held to the lines of csrc
that define them: a change of a block size, a threshold or a grid cap fails here instead of quietly moving a kernel's
variants and tails away from the shapes that were chosen to reach them.  Constants only, read from the sources' text; and,
from the same arithmetic the GPU cases assert, which variants and tails their shapes reach."""
import os
import re

import numpy as np

import grail_hip as G
import limit_stream_model as limit_stream
import resample_stream_model as resample_stream
import test_fir_gpu as fir
import test_levels_gpu as levels
import test_limit_stream_gpu as limit_stream_gpu
import test_limiter_gpu as limiter
import test_mix_gpu as mix
import test_resample_gpu as resample
import test_resample_stream_gpu as resample_stream_gpu
import test_stream_long_run_gpu as long_run
from test_limiter_host import detector

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


# ---- the stream kernels ----------------------------------------------------------------------------------------------------------
def test_the_resample_streams_chunk_and_the_passes_of_one():
    text, plan = source("resample_kernels.hip"), source("resample_plan.h")
    assert re.search(r"constexpr uint32_t RESAMPLE_STREAM_CHUNK = GRAIL_RESAMPLE_CHUNK;", plan)
    assert re.search(r"constexpr uint32_t RS_STREAM_PASSES = RESAMPLE_STREAM_CHUNK / RS_THREADS;", text)
    threads = constant(text + source("kernels.h"), "RS_THREADS")
    assert threads == resample_stream_gpu.PASS == 256 and G.RESAMPLE_CHUNK // threads == 4 and resample_stream_gpu.CHUNK == G.RESAMPLE_CHUNK
    # one instantiation of rs_outputs per count of passes, 1 ... 4, under every <STAGED, VEC, TAB>
    call = r"\s*rs_outputs<STAGED, VEC, TAB, %s>\([^;]*;\n"
    assert re.search(r"const uint32_t passes = \(count \+ RS_THREADS - 1u\) / RS_THREADS;[^\n]*\n\s*if \(passes <= 1u\)\n" + call % "1" +
                     r"\s*else if \(passes == 2u\)\n" + call % "2" + r"\s*else if \(passes == 3u\)\n" + call % "3" +
                     r"\s*else\n" + call % "RS_STREAM_PASSES", text)
    assert len(re.findall(r"rs_outputs<", text)) == 4


def passes_of(count):
    """the NPASS of every chunk of a call of `count` outputs that has outputs"""
    return {-(-min(resample_stream_gpu.CHUNK, count - m0) // resample_stream_gpu.PASS) for m0 in range(0, count, resample_stream_gpu.CHUNK)}


def stream_variants(pair, row_splits, stride=None, out_stride=None, in_offset=0, out_offset=0, tail_stride=None):
    """the (resample_stream_kernel<STAGED, VEC, TAB>, NPASS) that test_resample_stream_gpu.py's stream_rows starts for rows fed
    as row_splits say under a layout of its feed and flush: VEC by launch_resample_stream's rule, the finishing call's from
    out alone (it has no input)"""
    U, D, P = G.resample_ratio(*pair)
    n_calls = max(len(s) for s in row_splits)
    reached = set()
    fed = [0] * len(row_splits)
    for c in range(n_calls):
        ns = [s[c] if c < len(s) else 0 for s in row_splits]
        in_stride = stride or (max(ns + [1]) + 63) // 64 * 64
        o_stride = (resample_stream.ceil_div(in_stride * U, D) + 3) // 4 * 4 if out_stride is None else out_stride
        aligned = in_offset % 4 == 0 and out_offset % 4 == 0 and in_stride % 4 == 0 and o_stride % 4 == 0
        for i, n in enumerate(ns):
            reached |= {(resample.variant(U, D, P, aligned), k) for k in passes_of(resample_stream.stream_len(fed[i], n, U, D, P))}
            fed[i] += n
    t_stride = (resample_stream_gpu.tail_room(pair) + 7) // 4 * 4 if tail_stride is None else tail_stride
    aligned = out_offset % 4 == 0 and t_stride % 4 == 0
    for N in fed:
        reached |= {(resample.variant(U, D, P, aligned), k) for k in passes_of(resample_stream.stream_len(N, 0, U, D, P, finishing=True))}
    return reached


# what the seeds of test_every_split_gives_the_one_shot_row and the shapes of test_every_layout_gives_the_same_bits leave out
# of the forty: found by the arithmetic below, and the reason for test_calls_of_two_three_and_four_passes
MISSED_BY_THE_SPLITS = [(("staged", False, "global"), 2), (("staged", False, "lds"), 2), (("staged", False, "uniform"), 2),
                        (("unstaged", False, "global"), 2), (("unstaged", False, "uniform"), 3)]


def test_the_stream_suite_reaches_every_variant_of_the_resample_stream_kernel_under_every_count_of_passes():
    compiled = {(v, k) for v in resample.VARIANTS for k in (1, 2, 3, 4)}
    assert len(compiled) == 40
    by_splits = set()
    for pair in resample_stream_gpu.PAIRS:
        by_splits |= stream_variants(pair, resample_stream_gpu.every_split_rows(pair)[1])
    for pair in resample_stream_gpu.LAYOUT_PAIRS:
        row_splits, layouts = resample_stream_gpu.layout_splits(pair)
        for layout in layouts:
            by_splits |= stream_variants(pair, row_splits, **layout)
    assert by_splits <= compiled and {v for v, _ in by_splits} == set(resample.VARIANTS)
    assert {k for _, k in by_splits} >= {1, 4}
    assert sorted(compiled - by_splits) == sorted(MISSED_BY_THE_SPLITS)
    # the deterministic calls: every variant under two, three and four passes, whatever the seeds above give
    by_calls = set()
    for pair in resample_stream_gpu.LAYOUT_PAIRS:
        split, counts = resample_stream_gpu.pass_calls(pair)
        assert [sorted(passes_of(c)) for c in counts] == [[2], [3], [4]]
        by_calls |= stream_variants(pair, [split]) | stream_variants(pair, [split], in_offset=1, out_offset=1)
    assert by_calls >= {(v, k) for v in resample.VARIANTS for k in (2, 3, 4)}
    assert by_splits | by_calls == compiled


def test_the_advance_kernels_gather_a_calls_chunks_64_to_a_lap():
    """one lane per chunk and `c += 64u`: a call of 65 chunks or more sends lane 0 round again, which the long calls of
    test_stream_long_run_gpu.py do (their builders assert the chunk each planted sample falls in)"""
    for name, kernel, chunk in (("fir_kernels.hip", "fir_stream_advance_kernel", r"r\.count \+ FIR_CHUNK - 1u\) / FIR_CHUNK"),
                                ("resample_kernels.hip", "resample_stream_advance_kernel",
                                 r"r\.count \+ RESAMPLE_STREAM_CHUNK - 1u\) / RESAMPLE_STREAM_CHUNK"),
                                ("limiter_kernels.hip", "limit_stream_advance_kernel", r"sg\.count \+ LIMIT_CHUNK - 1u\) / LIMIT_CHUNK")):
        text = source(name)
        body = text[text.index("void " + kernel + "("):]
        assert re.search(r"const uint32_t chunks = \w+\.count \? \(" + chunk + r" : 1u;", body), name
        assert len(re.findall(r"for \(uint32_t c = lane; c < chunks; c \+= 64u\)", body)) == 1, name
        assert len(re.findall(r"c \+= 64u", text)) == 1, name
    assert long_run.LAPS == 65
    long_run.lapped_filter_case()
    long_run.lapped_resample_case()
    for hot in long_run.LAPPED_HOT.values():
        long_run.lapped_limit_case(hot)


def test_the_rows_that_cross_2_to_the_32_and_their_stand_ins():
    """the builders of test_stream_long_run_gpu.py assert where the calls end, where the samples that are not finite lie and
    why M zeros stand for N0; here also that the counts are 64 bits wide in the state the kernels read"""
    for name, state in (("fir_kernels.hip", r"struct FirStreamRow \{\n\s*uint64_t fed;"),
                        ("resample_kernels.hip", r"struct RsStreamRow \{\n\s*uint64_t fed, i;"),
                        ("limiter_kernels.hip", r"struct LimitStreamGroup \{\n\s*uint64_t fed, first;")):
        assert re.search(state, source(name)), name
    _, N0, calls, _, _ = long_run.long_filter_case()
    assert N0 < 1 << 32 < N0 + sum(calls[:2])
    for pair in long_run.LONG_PAIRS:
        long_run.long_resample_case(pair)
    for ell in long_run.LONG_ELLS:
        long_run.long_limit_case(ell)


def limit_stream_paths(ell, group, aligned, fed, n):
    """the data-dependent paths of limit_stream_kernel that a `next` call of n samples takes for a group fed `fed` before it,
    by the kernel's own arithmetic, chunk by chunk"""
    L, T = 1 << ell, G.LIMIT_CHUNK
    first = limit_stream.known(fed, ell)
    count = limit_stream.stream_len(fed, n, ell)
    if n == 0:
        return set()
    if count == 0:
        return {"count == 0, group of %d" % group}
    paths = set()
    for m0 in range(0, count, T):
        a = first + m0 - (L - 1)
        o = a - (a & 3) - 12
        paths.add("seam < 0" if fed - o < 0 else "seam >= 0")
        if fed > limit_stream.ring_capacity(ell):
            paths.add("oldest > 0")
        if aligned:
            paths.add("in_vec" if fed % 4 == 0 else "not in_vec")
    return paths


def test_the_limit_stream_kernels_paths_and_the_calls_that_take_them():
    text = source("limiter_kernels.hip")
    for line in (r"const bool in_vec = VEC && \(sg\.fed & 3u\) == 0u;", r"const int64_t seam = \(int64_t\)sg\.fed - o;",
                 r"const uint64_t skip = seam < 0 \? \(uint64_t\)\(-seam\) : 0u;", r"if \(count == 0u\) \{\n\s*for \(uint32_t j = 0; j < group; \+\+j\)",
                 r"const int64_t oldest = sg\.fed > ring_cap \? \(int64_t\)\(sg\.fed - ring_cap\) : 0;",
                 r"const bool work = __syncthreads_or\(hot \? 1 : 0\) != 0;", r"const int64_t a = \(int64_t\)t0 - \(int64_t\)\(L - 1u\);",
                 r"const int64_t o = a - \(int64_t\)sh - 12;"):
        assert re.search(line, text), line

    def walk(ell, group, aligned, split):
        paths, fed = set(), 0
        for n in split:
            paths |= limit_stream_paths(ell, group, aligned, fed, n)
            fed += n
        return paths

    # test_layout_and_neighbours, its aligned layout: calls of 4 k and 4 k + 1 samples, N above the ring of 64
    assert limit_stream_gpu.LAYOUTS["aligned"] == dict(stride=2048) and limit_stream.ring_capacity(3) == 64
    assert walk(3, 1, True, [400, 401, 403, 796]) == {"seam >= 0", "oldest > 0", "in_vec", "not in_vec"}
    # test_any_split_gives_the_one_shot_bits, its first split: everything at once, three chunks
    for ell in (0, 3, 8, 10):
        assert walk(ell, 1, True, [2 * G.LIMIT_CHUNK + 37]) == {"seam >= 0", "seam < 0", "in_vec"}
    # test_a_pair_fed_less_than_its_delay_counts_both_members: what no case reached with a group of two
    ell, _, split = limit_stream_gpu.pair_short_of_its_delay()
    assert "count == 0, group of 2" in walk(ell, 2, True, split)
    assert "count == 0, group of 2" not in walk(2, 2, True, [40]) | walk(0, 2, True, [116, 117]) | walk(6, 2, True, [211, 211])
    # test_under_the_ceiling_the_input_comes_back_delayed: no number above the ceiling anywhere, so `work` is false
    for ell in (0, 8):
        x = np.random.default_rng(780 + ell).uniform(-0.2, 0.2, 3000).astype(np.float32)
        assert detector(x)[0].max() < float(limit_stream_gpu.CEILING)
    # the rows that cross 2^32: the call behind the one that leaves N odd runs the VEC kernel with in_vec false
    N0, calls = long_run.data_calls(G.LIMIT_CHUNK)
    assert limit_stream_paths(10, 2, True, N0 + sum(calls[:2]), calls[2]) == {"seam >= 0", "oldest > 0", "not in_vec"}
    assert limit_stream_paths(10, 2, True, N0 + sum(calls[:4]), calls[4]) == {"seam >= 0", "seam < 0", "oldest > 0", "in_vec"}


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
