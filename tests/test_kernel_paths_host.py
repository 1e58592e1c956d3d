"""The constants that the path-coverage cases of the GPU suite mirror (tests/KERNEL_PATHS.md), held to the lines of csrc
that define them: a change of a block size, a threshold or a grid cap fails here instead of quietly moving a kernel's
variants and tails away from the shapes that were chosen to reach them.  Constants only, read from the sources' text; and,
from the same arithmetic the GPU cases assert, which variants and tails their shapes reach: for the recursive filters and the
dynamics, that the named cases reach exactly the compiled instantiations, and which of them nothing reached before."""
import os
import re

import numpy as np

import dyn_model
import grail_hip as G
import limit_stream_model as limit_stream
import resample_stream_model as resample_stream
import test_dyn_footprint_gpu as dyn_footprint
import test_dyn_gpu as dyn
import test_dyn_stream_gpu as dyn_stream
import test_fir_gpu as fir
import test_iir_blocked_code_objects as blocked_objects
import test_iir_blocked_gpu as iir_blocked
import test_iir_code_objects as iir_objects
import test_iir_gpu as iir
import test_iir_stream_gpu as iir_stream
import test_levels_gpu as levels
import test_limit_stream_gpu as limit_stream_gpu
import test_limiter_gpu as limiter
import test_mix_gpu as mix
import test_resample_gpu as resample
import test_resample_stream_gpu as resample_stream_gpu
import test_stream_long_run_gpu as long_run
import test_track_dyn_footprint_gpu as track_footprint
import test_track_dyn_gpu as track
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
    assert len(rows) > 170
    defined = {}
    for line in rows:
        ids = re.findall(r"`(test_\w+\.py)::(test_\w+)", line.rstrip().rstrip("|").split("|")[-1])
        assert ids, "a line without a test id: " + line
        for name, test in ids:
            if name not in defined:
                with open(os.path.join(ROOT, "tests", name)) as f:
                    defined[name] = set(re.findall(r"^def (test_\w+)\(", f.read(), re.M))
            assert test in defined[name], (name, test)


# ---- the recursive filters and the dynamics: iir_kernels.hip, biquad_block_kernels.hip, dyn_kernels.hip, track_env_kernels.hip ------
def pad64(n):
    return (max(n, 1) + 63) // 64 * 64


def test_the_tiles_blocks_and_unrolls_of_the_recursive_filters_and_the_dynamics():
    common, plan, dyn_plan = source("loudness_common.h"), source("iir_plan.h"), source("dyn_plan.h")
    assert constant(common, "LOUD_T") == constant(common, "LOUD_ROWS") == iir.TILE == 64
    assert constant(plan, "IIR_BLOCK") == iir_blocked.BLOCK == 1024 and constant(plan, "IIR_BLOCK_LANES") == 64
    assert constant(dyn_plan, "TRACK_TILE") == track.T == 1024 and constant(dyn_plan, "TRACK_WORKERS") == track.T // 4
    for name in ("iir_kernels.hip", "biquad_block_kernels.hip", "dyn_kernels.hip"):
        text = source(name)
        assert constant(text, "UNROLL") == 4, name
        assert len(re.findall(r"for \(; i \+ UNROLL <= run; i \+= UNROLL\)", text)) == 1, name
        assert len(re.findall(r"#pragma unroll 1\n\s*for \(; i < run; \+\+i\)", text)) == 1, name
    chain = source("track_env_kernels.hip")
    assert constant(chain, "H") == 8
    assert re.search(r"for \(; i \+ 2u \* H <= run; i \+= 2u \* H\)", chain) and re.search(r"#pragma unroll 1\n\s*for \(; i < run; \+\+i\)", chain)
    assert re.search(r"buf\[\(i \+ 2u \* H \+ q\) & \(TRACK_TILE - 1u\)\]", chain)              # the look-ahead that wraps
    # the lengths the track cases walk: a chain of fewer than sixteen, of sixteens and a remainder, of a whole tile
    runs = {n % track.T or (track.T if n else 0) for n in track.LENGTHS} | {track.T for n in track.LENGTHS if n > track.T}
    assert {1, 63, 65, 5, track.T - 1, track.T} <= runs and any(r < 16 for r in runs) and any(r > 16 and r % 16 for r in runs)
    assert sorted({-(-n // track.T) for n in track.LENGTHS}) == [0, 1, 2, 3, 4, 6]                # tiles: none, fill, full, drain


def test_the_bound_dispatch_and_the_vec_rules_of_the_four_launchers():
    dispatch = (r"if \(bound <= 1u\)\n\s*%s<1, %s>\(.*\n\s*else if \(bound == 2u\)\n\s*%s<2, %s>\(.*\n\s*else if \(bound <= 4u\)\n"
                r"\s*%s<4, %s>\(.*\n\s*else\n\s*%s<8, %s>\(")
    text = source("iir_kernels.hip")
    assert re.search(dispatch % (("iir_launch_vec", "STREAM") * 4), text)
    assert re.search(r"const bool vec = aligned16\(args\.rows, args\.row_stride, args\.out, args\.out_stride\);\n\s*if \(args\.state\)", text)
    text = source("biquad_block_kernels.hip")
    assert re.search(dispatch % (("block_launch_vec", "OUT") * 4), text)
    assert re.search(r"if \(bound <= 1u\)\n\s*hipLaunchKernelGGL\(biquad_block_propagate_kernel<1>.*\n\s*else if \(bound == 2u\)\n.*<2>.*\n"
                     r"\s*else if \(bound <= 4u\)\n.*<4>.*\n\s*else\n.*<8>", text)
    assert re.search(r"const bool vec = aligned16\(a\.rows, a\.row_stride\) && \(!OUT \|\| aligned16\(a\.out, a\.out_stride\)\);", text)
    assert re.search(r"if \(args\.n_rows == 0 \|\| args\.grid_blocks < 2u\) return hipSuccess;", text)
    keyed = (r"const bool vec = aligned16\(args\.rows, args\.row_stride, args\.out, args\.out_stride\) && "
             r"\(!args\.key \|\| aligned16\(args\.key, args\.key_stride\)\);")
    assert re.search(keyed + r"\n\s*if \(args\.state\)", source("dyn_kernels.hip"))
    assert re.search(keyed + r"\n\s*if \(args\.key\)", source("track_env_kernels.hip"))
    assert re.search(r"inline bool aligned16\(const void \*rows, uint64_t stride\) \{ return \(reinterpret_cast<uintptr_t>\(rows\) & 15u\) == 0 && "
                     r"\(stride & 3u\) == 0; \}", source("kernels.h"))
    # a set's bound is a power of two already (iir_set_image), and a keyed stream's call of no samples brings no key
    assert re.search(r"uint32_t b = 1;\n\s*while \(b < most\) b <<= 1;\n\s*\*bound = b;", source("iir_plan.cpp"))
    assert re.search(r"if \(ds->n_keys && in_stride\)", source("transform_streams.cpp"))
    assert [iir.bound_of([np.zeros((S, 5))]) for S in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    # the compiled sets are the ones the code-object tests enumerate
    assert sorted(iir.VARIANTS) == sorted((sb, bool(v), bool(s)) for sb in iir_objects.BOUNDS for v in (0, 1) for s in (0, 1))
    assert sorted(iir_blocked.VARIANTS, key=str) == sorted([("block", sb, bool(v), bool(o)) for sb in blocked_objects.BOUNDS for v in (0, 1)
                                                            for o in (0, 1)] + [("propagate", sb) for sb in blocked_objects.BOUNDS], key=str)
    assert len(iir.VARIANTS) == 16 and len(iir_blocked.VARIANTS) == 20 and len(dyn.VARIANTS) == 8 and len(track.VARIANTS) == 4


def sets_bound(sections):
    return iir.bound_of([np.zeros((S, 5)) for S in sections])


# What the suite launched before the cases named in tests/KERNEL_PATHS.md's sections for these four units were added: every
# call of the GPU modules as they stood, as (the sections of the set's filters, the layouts the case passes to its `run`; {}
# is the helper's own layout, aligned bases and strides of multiples of 64).
IIR_ROWS_BEFORE = [
    ((1, 2, 3), [{}]),                                                                   # test_row_counts
    ((2,), [{}]),                                                                        # test_lengths_either_side_of_a_tile
    ((3, 1), [{}, dict(stride=128, out_stride=192)]),                                    # test_a_wave_of_every_length_...
    ((2, 5), [dict(stride=304, out_stride=384)] + list(iir.SCALAR_LAYOUTS)),             # test_the_scalar_path_... on its one set
    ((2,), [dict(out_stride=s) for s in (100, 101, 128, 129, 217)] + [dict(stride=200, out_stride=0)]),     # test_out_stride_cuts_...
    ((2, 4), [{}]),                                                                      # test_tails
    ((1,), [{}]), ((2,), [{}]),                                                          # test_a_decay_through_the_denormals_...
    (tuple(range(1, 9)), [{}]), ((1,), [{}]), ((1, 2), [{}]), ((1, 2, 3, 4), [{}]),      # test_one_wave_of_one_to_eight_sections
    ((2, 1, 3), [{}]),                                                                   # test_filter_per_row_none_and_outside_the_set
    ((2,), [{}, dict(out_stride=32)]),                                                   # test_nonfinite_samples_...
    ((2, 1), [{}]),                                                                      # test_an_unstable_filter_...
    ((3, 8, 1), [{}]),                                                                   # test_a_rows_bits_do_not_depend_on_where_it_lies
]
# (sections, the Feeder's in_stride, out_stride, in_offset, out_offset): next and finish
IIR_STREAMS_BEFORE = [
    (tuple(range(1, 9)), 704, 704, 0, 0), (tuple(range(1, 9)), 701, 703, 1, 3),          # test_any_split_gives_the_one_shot_rows
    ((1, 2), 704, 704, 0, 0),                                                            # test_finish_on_some_rows_...
    ((4,), 128, 128, 0, 0),                                                              # test_a_row_fed_nothing_...
]
# (sections, row_stride, tail, layouts)
BLOCKED_BEFORE = [
    ((1, 3, 8), 70016, 0, [{}]), ((1, 3, 8), 70016, 7, [{}]), ((1, 3, 8), 70016, 1500, [{}]),       # test_rows_either_side_...
    ((1, 3, 8), 70016, 7, [dict(in_offset=1, stride=70001, out_offset=1, out_stride=70011), dict(in_offset=1), dict(stride=70003),
                           dict(out_offset=3), dict(out_stride=70009)]),                 # test_the_scalar_path_gives_the_aligned_paths_bits
    ((2, 4), 5056, 100, [dict(out_stride=s) for s in (2500, 2049, 1024, 5050, 0)]),      # test_cuts_counts_refusals_and_canaries
    ((8,), 70016, 16, [{}]), ((1, 2), 3008, 16, [{}]),                                   # test_scratch_left_by_a_longer_call
    ((4, 1, 8, 1), 70016, 0, [{}]), ((4, 1, 8, 1), 70016, 300, [{}]),                    # test_against_the_serial_call_on_the_device
    ((2,), pad64((1 << 20) + 3), 5, [{}]), ((8,), pad64((1 << 20) + 3), 5, [{}]),        # test_one_long_row
]
MISSED_BEFORE = {
    # no scalar call on a set of bound 1 or 4 (bound 2's came from out_stride 101, 129 and 217 of the cutting case, not from
    # the scalar-path case, whose one set has bound 8), and no stream of bound 1 at all nor a scalar one below 8
    "iir": [(1, False, False), (1, False, True), (1, True, True), (2, False, True), (4, False, False), (4, False, True)],
    # no set of bound 1, and the 4-byte kernels of bounds 2 and 4 but for <4, false, true>: the output pass of the cutting
    # case's out_stride of 2 049 and 5 050
    "blocked": [("block", 1, False, False), ("block", 1, False, True), ("block", 1, True, False), ("block", 1, True, True),
                ("block", 2, False, False), ("block", 2, False, True), ("block", 4, False, False), ("propagate", 1)],
    # all eight and all four ran: test_dyn_footprint_gpu.py and test_track_dyn_footprint_gpu.py walk them by name, and the
    # stream case's strides of max(feed) + call are of both kinds.  What was missed there is paths, below
    "dyn": [],
    "track": [],
}
# (of a stream's calls that another call follows: the footprint case's streams, out_stride 203 at in_stride 201, end with their
# first call, so nothing reads what it saved)
DYN_STREAM_PATHS_MISSED_BEFORE = ["in_len above in_stride", "out_stride above in_stride", "the key alone misaligned", "alphas of 0",
                                  "an envelope below 2^-32 carried from call to call"]


def layout_variant(variant, bound, default_stride, default_out_stride, kw, **more):
    return variant(bound, kw.get("in_offset", 0), kw.get("stride", default_stride), kw.get("out_offset", 0),
                   kw.get("out_stride", default_out_stride), **more)


def iir_reached(rows_cases, stream_cases):
    reached = set()
    for sections, layouts in rows_cases:
        reached |= {layout_variant(iir.variant, sets_bound(sections), 64, 64, kw) for kw in layouts}
    for sections, in_stride, out_stride, in_offset, out_offset in stream_cases:
        reached.add(iir.variant(sets_bound(sections), in_offset, in_stride, out_offset, out_stride, True))
        reached.add(iir.variant(sets_bound(sections), 0, 0, out_offset, out_stride, True))               # the finishing call
    return reached


def test_the_iir_cases_reach_every_instantiation_of_the_kernel():
    compiled = set(iir.VARIANTS)
    before = iir_reached(IIR_ROWS_BEFORE, IIR_STREAMS_BEFORE)
    assert before <= compiled and sorted(compiled - before) == sorted(MISSED_BEFORE["iir"]) and MISSED_BEFORE["iir"]
    # the scalar-path case under every bound, with its smallest strides; the stream case under every bound and both layouts
    short = [dict(stride=1, out_stride=75), dict(stride=1, out_stride=72), dict(stride=4, out_stride=76), dict(stride=4, out_stride=75)]
    rows_now = [(iir.SCALAR_SECTIONS[most], [dict(stride=304, out_stride=384)] + list(iir.SCALAR_LAYOUTS) + short) for most in iir.BOUNDS]
    streams_now = [(iir_stream.BOUND_SECTIONS[most], kw["in_stride"], kw["out_stride"], kw.get("in_offset", 0), kw.get("out_offset", 0))
                   for most in iir.BOUNDS for kw in iir_stream.BOUND_LAYOUTS.values()]
    assert [sets_bound(iir.SCALAR_SECTIONS[m]) for m in iir.BOUNDS] == [sets_bound(iir_stream.BOUND_SECTIONS[m]) for m in iir.BOUNDS] == list(iir.BOUNDS)
    reached = iir_reached(rows_now, streams_now)
    assert reached == compiled                                                          # by the two cases alone
    assert set(MISSED_BEFORE["iir"]) <= reached
    # the stream case's calls: a lane that pauses while its wave runs 63 steps and whole tiles, and 65 rows are a wave and one
    for most in iir.BOUNDS:
        rows, filters, which = iir_stream.bound_case(most)
        calls = iir_stream.bound_calls(rows)
        assert len(rows) == 65 and all(60 <= len(x) <= 200 for x in rows) and len({len(x) for x in rows}) > 30
        assert [int(c.max()) for c in calls[:2]] == [63, 1] and (calls[0] == 0).sum() == 9 and calls[2].max() > 128
        assert sets_bound([len(np.asarray(f).reshape(-1, 5)) for f in filters]) == most


def blocked_reached(cases):
    reached = set()
    for sections, stride, tail, layouts in cases:
        for kw in layouts:
            out_stride = kw.get("out_stride", pad64(stride + tail))
            reached |= layout_variant(iir_blocked.variant, sets_bound(sections), stride, out_stride, kw, tail=tail)
    return reached


def test_the_blocked_cases_reach_every_instantiation_of_the_kernels():
    compiled = set(iir_blocked.VARIANTS)
    before = blocked_reached(BLOCKED_BEFORE)
    assert before <= compiled and sorted(compiled - before, key=str) == sorted(MISSED_BEFORE["blocked"], key=str) and MISSED_BEFORE["blocked"]
    lower = [(tuple(len(f) for f in iir_blocked.edge_rows(bound)[0]), 65600, tail, [dict(out_stride=66624)] + [kw for kw in iir_blocked.BOUND_LAYOUTS.values() if kw])
             for bound in (1, 2, 4) for tail in iir_blocked.BOUND_TAILS]
    eight = BLOCKED_BEFORE[:4]                           # test_rows_either_side_... and test_the_scalar_path_..., as they stand
    assert [sets_bound(c[0]) for c in lower] == [1, 1, 2, 2, 4, 4] and {sets_bound(c[0]) for c in eight} == {8}
    reached = blocked_reached(lower + eight)
    assert reached == compiled                                                          # by the three cases alone
    assert set(MISSED_BEFORE["blocked"]) <= blocked_reached(lower)
    # the workgroup that starts past the stride: block 64 of a row of 65 536 samples in a stride of as many
    assert 64 * iir_blocked.BLOCK > 65536 - 4 and all(pad64(n) - 4 > n // (64 * 1024) * 64 * 1024 for n in (65537, 70000, (1 << 20) + 3))


def dyn_reached_by_the_footprints():
    reached = set()
    for stream, keyed, shape in dyn_footprint.CASES:
        stride, offset, out_stride = dyn_footprint.SHAPES[shape]
        out_offset = dyn_footprint.GUARD_ROWS * out_stride + offset
        reached.add(dyn.variant(offset, stride, out_offset, out_stride, keyed, offset, stride, stream))
    return reached


def test_the_dynamics_cases_reach_every_instantiation_of_the_kernel_and_the_stream_paths_they_missed():
    compiled = set(dyn.VARIANTS)
    reached = dyn_reached_by_the_footprints()
    assert reached == compiled and sorted(compiled - reached) == MISSED_BEFORE["dyn"] == []
    # the stream case as it stood: both paths under either kind of key, by its strides of max(feed) + call alone
    old = set()
    facts = {"in_len above in_stride": False, "out_stride above in_stride": False, "the key alone misaligned": False}
    for keyed in (False, True):
        rows = dyn_stream.corpus(keyed)[0]
        for feed, stride in dyn_stream.chunking_calls([len(x) for x in rows]):
            old.add(dyn.variant(0, stride, 0, stride, keyed, 0, stride, True))          # (in, out and key at the one stride)
            facts["in_len above in_stride"] |= max(feed) > stride
    assert old == {v for v in compiled if v[2]}
    curves = dyn.three_curves()
    facts["alphas of 0"] = any(a == 0.0 for c in curves for a in c[1])
    rows, which, _, _ = dyn_stream.corpus(False)
    model, at, low = dyn_model.DynStreamModel(curves, which), [0] * len(rows), False
    for feed, _ in dyn_stream.chunking_calls([len(x) for x in rows]):
        model.next([x[a:a + f] for x, a, f in zip(rows, at, feed)])
        at = [a + f for a, f in zip(at, feed)]
        low |= bool(np.any((model.e > 0.0) & (model.e < 2.0 ** -32)))
    facts["an envelope below 2^-32 carried from call to call"] = low
    assert sorted(k for k, v in facts.items() if not v) == sorted(DYN_STREAM_PATHS_MISSED_BEFORE)
    # the cases that take them now, by their own arguments
    key_only = dyn_stream.KEY_LAYOUTS["key base"][0]
    assert key_only.get("in_offset", 0) == 0 and key_only["in_stride"] % 4 == 0 and key_only["out_stride"] % 4 == 0 and key_only["key_offset"] == 1
    assert dyn_stream.KEY_LAYOUTS["key stride"][0]["key_stride"] % 2 == 1 and dyn_stream.KEY_LAYOUTS["rows base"][0]["key_stride"] % 4 == 0
    assert sum(1 for c in dyn.edge_curves() if tuple(c[1]) == (0.0, 0.0)) == 2
    dyn_stream.edge_calls(len(dyn.edge_samples()))


def test_the_track_cases_reach_every_instantiation_of_the_kernel():
    compiled = set(track.VARIANTS)
    T = track.T
    wide, odd, ks = 2 * T + 64, 2 * T + 9, 2 * T + 320
    # test_the_scalar_path_gives_the_aligned_paths_bits, and the last two calls of test_keys_that_end_inside_a_tile_...
    reached = {track.variant(0, wide, 0, wide), track.variant(1, odd, 1, odd), track.variant(0, odd, 0, wide),
               track.variant(0, pad64(2 * T + 300), 0, pad64(2 * T + 300), True, 0, ks), track.variant(0, pad64(2 * T + 300), 0, pad64(2 * T + 300), True, 1, ks + 1)}
    assert reached == compiled and sorted(compiled - reached) == MISSED_BEFORE["track"] == []
    by_footprint = set()
    for keyed, shape in track_footprint.CASES:
        stride, offset, out_stride = track_footprint.SHAPES[shape]
        by_footprint.add(track.variant(offset, stride, track_footprint.GUARD_ROWS * out_stride + offset, out_stride, keyed, offset, stride))
    assert by_footprint == compiled
