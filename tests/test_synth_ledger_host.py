"""The ledger of the synthesis kernels (tests/synth_ledger.py) against the built library and against its own corpora,
without a GPU.  The names built from the synth_kernel and scan_kernel symbols in the gfx950 code objects of
libgrail_hip.so EQUAL the names in the ledger: an instantiation compiled without a cell fails here and is named, and so
does a cell for a kernel that is not compiled.  The ledger has no "unreachable" status: a kernel no sequence of public
calls can launch is not to be compiled (csrc/synth_launch_impl.h decides with `if constexpr` which instantiations a unit
holds).  tests/SYNTH_KERNELS.md has one line per entry, and every corpus has, among the rows a cell takes, the rows the
cell relies on — checked from the oracle's rows and the corpus' own inputs alone."""
import os
import re

import numpy as np
import pytest

import footprint as F
import grail_hip as G
import synth_ledger as SL
from test_code_objects import kernels  # noqa: F401  (the fixture: {kernel symbol: metadata} of the library's code objects)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_compiled_instantiations_are_the_ledgers(kernels):  # noqa: F811
    compiled = SL.names_of_symbols(kernels)
    assert len(compiled) >= 60
    no_cell = sorted(set(compiled) - set(SL.BY_NAME))
    no_kernel = sorted(set(SL.BY_NAME) - set(compiled))
    assert not no_cell and not no_kernel, (
        f"compiled without a cell in tests/synth_ledger.py: {[(n, compiled[n]) for n in no_cell]}; "
        f"cells whose kernel is not in the library: {no_kernel}")


def test_names_and_template_arguments_convert_both_ways():
    for e in SL.ENTRIES:
        args = SL.synth_args(e.name)
        if args is None:
            m = re.fullmatch(r"scan_kernel<pairs=(\d),(SPLIT,)?FAST>", e.name)
            assert m and SL.scan_name((int(m.group(1)), int(bool(m.group(2))))) == e.name
        else:
            assert len(args) == len(SL.SYNTH_ARGS) == 13 and SL.synth_name(args) == e.name
    # start()'s format, csrc/synth_kernel.h
    with open(os.path.join(ROOT, "grail-rs_amd", "csrc", "synth_kernel.h")) as f:
        text = f.read()
    assert '"synth_kernel<L=%d,T=%d,W=%d,%d,%s%s%sNFA=%d%s%s%s%s%s>"' in text
    assert SL.synth_name((4, 64, 4, 1, 1, 0, 1, 4, 1, 0, 4, 0, 0)) == "synth_kernel<L=4,T=64,W=4,1,STREAM,ANYBL,NFA=4,PIPE,R16>"
    assert SL.synth_name((1, 64, 1, 1, 0, 1, 1, 8, 0, 1, 2, 1, 1)) == "synth_kernel<L=1,T=64,W=1,1,HALF,ANYBL,NFA=8,FAST,SPLIT,MID>"
    sym = "_ZN5grail12_GLOBAL__N_111scan_kernelILi2ELb1EEEvNS_9SynthArgsE"
    assert SL.names_of_symbols([sym, "_ZN5grail12_GLOBAL__N_114lengths_kernelENS_7LenArgsE"]) == {"scan_kernel<pairs=2,SPLIT,FAST>": sym}


def test_every_line_of_the_readable_form_names_an_entry_and_every_entry_has_a_line():
    with open(os.path.join(ROOT, "tests", "SYNTH_KERNELS.md")) as f:
        rows = [line for line in f if line.startswith("| `")]
    named = [re.match(r"\| `([^`]+)` \|", line).group(1) for line in rows]
    assert len(named) == len(set(named)), "a kernel with two lines"
    assert set(named) == set(SL.BY_NAME), (sorted(set(named) - set(SL.BY_NAME)), sorted(set(SL.BY_NAME) - set(named)))
    for line in rows:
        assert len(line.rstrip().rstrip("|").split("|")) == 4, "three columns: " + line
    # (the table is markdown()'s: a changed cell shows in the readable form too)
    assert "".join(rows) == "".join(line + "\n" for line in SL.markdown().splitlines() if line.startswith("| `"))


def _csrc(name):
    with open(os.path.join(ROOT, "grail-rs_amd", "csrc", name)) as f:
        return f.read()


def test_the_rows_of_a_workgroup_are_the_launch_codes():
    """How many rows a workgroup of each cell's launch holds, by the lines of csrc that decide it (a changed rule fails
    here, not by quietly moving the cells off 'two workgroups, the last one partly filled'), and every cell's row count
    by those rules."""
    impl, pipe, cost, plan = _csrc("synth_launch_impl.h"), _csrc("synth_inst_pipe.hip"), _csrc("family_cost.cpp"), _csrc("launch_plan.h")
    assert "const uint32_t per_block = (64u / L) * WAVES;" in impl                                       # lane_grid
    assert impl.count("const dim3 grid(((args.n_utt + 63u) / 64u) * args.split_chunks), block(64);") == 2     # time-split
    for slots in (16, 8):                                                                                # launch_pipe4 / 8
        assert f"const uint32_t fill = args.pipe_fill != 0u && !args.state ? args.pipe_fill : {slots}u;" in pipe
    for line in ("if (!f.pipe || !ctx->opt.pipe_spread || !rows_differ(batch)) return 0u;",              # pipe_fill_for
                 "const uint32_t slots = f.live4 ? 16u : 8u;", "const uint32_t units = 2u * (uint32_t)ctx->cus;",
                 "const uint32_t fill = (rows + units - 1u) / units;", "return fill >= slots ? 0u : (fill < 1u ? 1u : fill);",
                 "return built && ((uint64_t)rows * (uint64_t)f.L + 63u) / 64u > ctx_simds(ctx);"):      # family_cohabits
        assert line in cost, line
    assert "inline uint64_t ctx_simds(const PlanEnv *ctx) { return 4ull * (uint64_t)ctx->cus; }" in plan
    # the mirror of pipe_fill_for: spread thin on a large device, every slot without the option or when resumable
    assert [SL.pipe_fill(19, 16, 256, 1, True, False), SL.pipe_fill(19, 16, 256, 0, True, False),
            SL.pipe_fill(19, 16, 256, 1, False, False), SL.pipe_fill(19, 16, 256, 1, True, True)] == [1, 16, 16, 16]
    assert [SL.pipe_fill(r, 16, 256, 1, True, False) for r in (512, 513, 7680, 7681)] == [1, 2, 15, 16]
    for e in SL.ENTRIES:
        args = SL.synth_args(e.name)
        if args is None:
            assert e.rows >= 2                                  # scan_kernel: dim3(args.n_utt), a workgroup per row
            continue
        L, waves, minw, stream, pipe_kernel = args[0], args[2], args[3], bool(args[4]), bool(args[8])
        if minw == 2:
            # more waves than the four SIMDs of the one compute unit the cell assumes
            assert e.options["assume_compute_units"] == 1 and e.options["two_waves_per_simd"] == 1, e.name
            assert (e.rows * L + 63) // 64 > 4 * e.options["assume_compute_units"], e.name
            continue
        if pipe_kernel:
            assert stream or e.options["pipeline_spread"] == 0, e.name
            # (whatever device the suite meets: one compute unit, an MI355X, a larger one)
            fills = {SL.pipe_fill(e.rows, 64 // L, cus, e.options.get("pipeline_spread", 1), True, stream) for cus in (1, 256, 1024)}
            assert fills == {{4: 16, 8: 8}[L]}, (e.name, fills)
            per_block = fills.pop()
        else:
            per_block = (64 // L) * waves
        assert e.rows == per_block + 3 and -(-e.rows // per_block) == 2, e.name


def test_forms_and_arithmetic_follow_from_the_names():
    assert {e.form for e in SL.ENTRIES} == {"f32", "i16", "batch-stream", "live-stream"}
    for e in SL.ENTRIES:
        args = SL.synth_args(e.name)
        assert bool(args and args[4]) == ("stream" in e.form), e.name                  # STREAM kernels, resumable launches
        tolerance = args is None or bool(args[9])        # FAST (SPLIT and MID kernels are FAST kernels), scan_kernel
        assert e.arithmetic == ("tolerance" if tolerance else "exact"), e.name
        assert not (e.form == "i16" and tolerance), e.name
        assert e.corpus in SL.CORPORA
        # (the time-split kernels take only the corpus' own stride: a capacity of 1021 gives no grid of two chunks)
        assert (1021 in e.launches) == ("stream" not in e.form and not (args and args[11])), e.name


def _cuts():
    """(corpus, rows) of every cell, with the entries that take it."""
    cuts = {}
    for e in SL.ENTRIES:
        cuts.setdefault((e.corpus, e.rows), []).append(e)
    return sorted(cuts.items())


@pytest.mark.parametrize("corpus,rows,entries", [pytest.param(c, r, es, id=f"{c}-{r}") for (c, r), es in _cuts()])
def test_the_corpus_has_the_rows_its_cells_rely_on(corpus, rows, entries):
    voices, segs, offs, vids, seeds, ref, ref_len, S = F.first_rows(SL.corpus(corpus), rows)
    lens = ref_len.astype(np.int64)
    assert len(lens) == rows
    assert set((lens % 4).tolist()) == {0, 1, 2, 3}
    assert np.any(lens < 64), "no row shorter than a 64-sample tile"
    assert S % 64 == 0 and lens.max() < S and np.isfinite(ref).all()
    assert len(set(lens.tolist())) > rows // 2                    # rows that differ in length
    n_segs = np.diff(offs.astype(np.int64))
    pow2 = np.log2(segs["blend_length"].astype(np.float64)) % 1 == 0
    amp = np.array([[list(p.formant_amp) for p in v.phonemes] for v in voices])       # [voice, phoneme, formant]
    upper_silent = bool(np.all(amp[:, :, 4:] == 0.0))
    lean_rows = (n_segs.min() >= 1 and segs["length"].min() * F.RATE >= 2.0 and
                 set(segs["phoneme"].tolist()) <= {G.PH_A, G.PH_E, G.PH_SILENCE})
    # what the corpus is, by its name
    assert upper_silent == (not corpus.startswith("live8")) and (upper_silent or bool(np.all(amp != 0.0)))
    assert pow2.all() == (not corpus.endswith("_anybl"))
    assert lean_rows == (not corpus.startswith("odd"))
    if corpus.startswith("odd"):
        # not `plain` to the planner both ways: a Stop or Glide phoneme, a segment shorter than two samples
        assert set(segs["phoneme"].tolist()) & {G.PH_STOP, G.PH_GLIDE} and segs["length"].min() * F.RATE < 2.0
        assert n_segs.min() == 0 and all(np.any(lens == k) for k in (0, 1, 2, 3))
    for e in entries:
        args = SL.synth_args(e.name)
        if "stream" in e.form:
            assert np.any(lens > sum(SL.PULLS)), e.name
            assert lens.max() > sum(SL.PULLS) + 2 * SL.REST, e.name               # several pulls of REST
        elif 1021 in e.launches:
            assert (lens > 1021).sum() >= 2 and (lens <= 1021).sum() >= 2, e.name      # cut rows beside whole ones
        if e.form == "live-stream":
            continue                # (a live stream's kernel does not depend on the segments: it is opened before they come)
        four = args[7] == 4 if args else "pairs=2" in e.name
        # four formants laid out: formants 5 - 8 silent and every row one the lean families take
        assert four == (upper_silent and lean_rows), e.name
        if args is None:
            continue                # (scan_kernel takes every blend length)
        stream, half, anybl, pipe, fast = args[4], args[5], args[6], args[8], args[9]
        if half and not anybl:
            assert upper_silent and not lean_rows and pow2.all(), e.name          # HALF alone: half-capable, powers of two
        elif half and not stream:
            assert not pow2.all(), e.name                                         # one-shot HALF,ANYBL: a blend that is no power of two
        elif half:
            assert not pow2.all() or upper_silent, e.name                         # resumable: any_blend or half_capable
        elif anybl and not (stream and (pipe or (fast and not four))):     # (those resumable kernels: ANYBL whatever the batch)
            assert not pow2.all(), e.name
        elif not anybl:
            assert pow2.all(), e.name
            assert four or not upper_silent, e.name                              # eight formants, no HALF: not half-capable
