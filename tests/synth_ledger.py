"""The ledger of the synthesis kernels: one entry per compiled instantiation of synth_kernel (csrc/synth_kernel.h) and of
scan_kernel (csrc/scan_kernels.hip) — the name grail_last_kernel_name prints for it, and the cell that launches it: the
launch form, the corpus, the options, the rows and the strides or pulls.  tests/test_synth_ledger_host.py holds the set
of names to the kernel symbols of the built library (both ways) and the corpora to the properties the cells rely on;
tests/test_synth_ledger_gpu.py runs every cell, asserts the whole name and holds the rows to the oracle.
tests/SYNTH_KERNELS.md is the readable form (markdown() below writes it).  A plain helper module: it holds no test and no
fixture, and nothing here needs a GPU.

Which instantiation a launch takes is decided in csrc/synth_launch_impl.h, csrc/synth_inst_*.hip and
csrc/scan_kernels.hip from args.state, live4, any_blend, half_capable, cohabit, fast, pipe and split_chunks; what sets
those is in csrc/synthesize.cpp (launch_block), csrc/streams.cpp and csrc/family_choice.cpp."""
import collections
import re

import numpy as np

import footprint as F
import grail_hip as G
import oracle_lib as O
from grail_hip import workload as W

# ---- names ---------------------------------------------------------------------------------------------------------------
SYNTH_ARGS = ("L", "T", "WAVES", "MINW", "STREAM", "HALF", "ANYBL", "NFA", "PIPE", "FAST", "PQP", "SPLIT", "MID")


def synth_name(args):
    """What start() of csrc/synth_kernel.h prints for the 13 template arguments (test_code_objects.py::_synth's tuple)."""
    L, T, waves, minw, stream, half, anybl, nfa, pipe, fast, pqp, split, mid = args
    return "synth_kernel<L=%d,T=%d,W=%d,%d,%s%s%sNFA=%d%s%s%s%s%s>" % (
        L, T, waves, minw, "STREAM," if stream else "", "HALF," if half else "", "ANYBL," if anybl else "", nfa,
        ",PIPE" if pipe else "", ",FAST" if fast else "", ",R16" if pqp == 4 else ",R32" if pqp == 8 else "",
        ",SPLIT" if split else "", ",MID" if mid else "")


def scan_name(args):
    """What csrc/synthesize.cpp launch_block records for scan_kernel<NP, SPLIT> (NP: formant pairs, 2 or 4)."""
    pairs, split = args
    return "scan_kernel<pairs=%d,%sFAST>" % (pairs, "SPLIT," if split else "")


def synth_args(name):
    """The 13 template arguments of a printed synth_kernel name (the inverse of synth_name), or None."""
    m = re.fullmatch(r"synth_kernel<L=(\d+),T=(\d+),W=(\d+),(\d+),(STREAM,)?(HALF,)?(ANYBL,)?NFA=(\d+)(,PIPE)?(,FAST)?(,R16|,R32)?"
                     r"(,SPLIT)?(,MID)?>", name)
    if not m:
        return None
    g = m.groups()
    pqp = {None: 2, ",R16": 4, ",R32": 8}[g[10]]
    return (int(g[0]), int(g[1]), int(g[2]), int(g[3]), int(bool(g[4])), int(bool(g[5])), int(bool(g[6])), int(g[7]),
            int(bool(g[8])), int(bool(g[9])), pqp, int(bool(g[11])), int(bool(g[12])))


def names_of_symbols(symbols):
    """{printed name: symbol} of the synth_kernel and scan_kernel instantiations among mangled kernel symbols."""
    out = {}
    for sym in symbols:
        m = re.search(r"(synth|scan)_kernelI((?:L[ib]\d+E)+)E", sym)
        if not m:
            continue
        args = tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2)))
        assert len(args) == (13 if m.group(1) == "synth" else 2), sym
        name = synth_name(args) if m.group(1) == "synth" else scan_name(args)
        assert name not in out, (name, sym, out[name])
        out[name] = sym
    return out


# ---- corpora -------------------------------------------------------------------------------------------------------------
# tests/footprint.py's four, and two more by the same recipe (footprint._segments) and oracle calls:
#   live8_anybl   eight live formants (the eight presets), blend lengths of 3 - 30 ms: none a power of two
#   odd_anybl     the half-capable voice (formants 5 - 8 silent in every phoneme) in a batch the four-formant kernels do not
#                 take (rows without segments, of 1 - 3 samples, zero-length segments, Stop and Glide), blend lengths that
#                 are no powers of two; `odd` is the same with power-of-two blend lengths
NEW_CORPORA = {"live8_anybl": (105, True, False, True), "odd_anybl": (106, False, True, True)}     # seed, presets, odd, any_blend
CORPORA = F.VARIANTS + tuple(NEW_CORPORA)
_cache = {}


def corpus(name):
    """(voices, segs, offs, vids, seeds, ref, ref_len, S) as footprint.corpus gives it: computed once, read-only."""
    if name in F.VARIANTS:
        return F.corpus(name)
    if name not in _cache:
        seed, presets, odd, any_blend = NEW_CORPORA[name]
        rng = np.random.default_rng(seed)
        voices = W.preset_voices(8) if presets else W.single_voice()
        utts = F._segments(rng, F.N_UTT, any_blend, odd)
        segs = G.segments([s for u in utts for s in u])
        offs = np.cumsum([0] + [len(u) for u in utts]).astype(np.uint32)
        vids = (np.arange(F.N_UTT) % len(voices)).astype(np.uint32)
        seeds = rng.integers(0, 2 ** 32, F.N_UTT, dtype=np.uint64).astype(np.uint32)
        lens = O.count_batch(F.ovoices(voices), segs, offs, vids, seeds)
        S = (int(lens.max()) + 63) // 64 * 64
        S += 64 if S == int(lens.max()) else 0
        ref, ref_len = O.synthesize_batch(F.ovoices(voices), segs, offs, vids, seeds, S)
        assert np.array_equal(ref_len, lens)
        for a in (segs, offs, vids, seeds, ref, ref_len):
            a.setflags(write=False)
        _cache[name] = (voices, segs, offs, vids, seeds, ref, ref_len, S)
    return _cache[name]


# ---- the table -----------------------------------------------------------------------------------------------------------
# form: "f32" / "i16" (one-shot; an i16 cell renders the f32 rows too, at every stride, and holds both), "batch-stream",
# "live-stream".  launches: the strides of a one-shot cell ("S": the corpus'
# own, nothing cut; 1021: cuts inside a tile, GRAIL_ERR_BUFFER_TOO_SMALL) or the quotas of a stream's first pulls (PULLS,
# then REST per pull until the stream ends).  arithmetic: "exact" (bit for bit) or "tolerance" (G.FAST_TOLERANCE x
# max(1, peak)).  route: the condition that takes a launch to this instantiation, for SYNTH_KERNELS.md.
Entry = collections.namedtuple("Entry", "name form corpus options rows launches arithmetic route")
PULLS, REST = (1, 63, 65), 2000
ONE_SHOT, UNCUT = ("S", 1021), ("S",)
TWO_WAVE_ROWS = F.N_UTT             # (what the footprint cells of the two-wave kernels take on a device assumed to have 4 SIMDs)
SCAN_ROWS = 24                      # one workgroup per row
EXACT = {"arithmetic": 0}
FAST = {"arithmetic": 1, "time_split": 0, "time_parallel_scan": 0}
TWO_WAVES = {"assume_compute_units": 1, "two_waves_per_simd": 1}
SPLIT = {"time_parallel_scan": 0, "time_split_min_utterances": 0, "composite_launches": 0, "time_split_chunks": 3}
SHAPE = {1: (32, 1), 2: (64, 1), 4: (32, 4), 8: (64, 4)}      # L: (T, WAVES) of the synth_inst_{exact,fast}_l*.hip units
ENTRIES = []


def per_block(args):
    """Rows per workgroup when every slot is taken: (64 / L) x WAVES for the lane kernels (synth_launch_impl.h lane_grid; the
    time-split kernels: 64 lanes per chunk), 64 / L for the pipelined workgroups, whose four waves share 16 (L = 4) or 8
    (L = 8) utterances (synth_inst_pipe.hip).  How many a pipelined workgroup of a launch really holds: pipe_fill."""
    L, waves, pipe = args[0], args[2], args[8]
    return 64 // L if pipe else (64 // L) * waves


def pipe_fill(rows, slots, compute_units, spread, ragged, resumable):
    """Utterances per pipelined workgroup of a launch of `rows` rows: csrc/family_cost.cpp pipe_fill_for (one-shot launches
    of rows that differ in length, "pipeline_spread" on: as few per workgroup as give every compute unit two workgroups) and
    launch_pipe4 / launch_pipe8 of csrc/synth_inst_pipe.hip (`slots` otherwise, and for resumable launches).  The one-shot
    PIPE cells switch "pipeline_spread" off: with it, 19 rows on 256 compute units are 19 workgroups of one utterance, and
    slots 1 ... 15 of a workgroup — what its waves share — are never taken."""
    if resumable or not spread or not ragged:
        return slots
    fill = -(-rows // (2 * compute_units))
    return slots if fill >= slots else max(fill, 1)


def _synth(args, form, corpus_name, options, route, launches=None, rows=None):
    stream = bool(args[4])
    tolerance = bool(args[9])
    if rows is None:
        rows = TWO_WAVE_ROWS if args[3] == 2 else per_block(args) + 3
    if launches is None:
        launches = PULLS if stream else UNCUT if args[11] else ONE_SHOT
    ENTRIES.append(Entry(synth_name(args), form, corpus_name, dict(options), rows, launches,
                         "tolerance" if tolerance else "exact", route))


def _lane_entries():
    # corpora by what the instantiation lays out and divides alpha by
    four = {0: "lean4", 1: "lean4_anybl"}
    eight = {0: "live8", 1: "live8_anybl"}
    for L, (T, waves) in SHAPE.items():
        pin = {"lanes_per_utterance": L}
        # -- exact, one-shot (synth_launch_impl.h launch_one_exact)
        if L <= 4:
            for anybl in (0, 1):
                _synth((L, 64 if L == 4 else T, waves, 1, 0, 0, anybl, 4, 0, 0, 2, 0, 0), "f32", four[anybl], dict(EXACT, **pin),
                       f"launch_one_exact<{L}>: `!args.state && args.live4`, `args.any_blend` {'set' if anybl else 'clear'}"
                       + (" (T4 = 64)" if L == 4 else ""))
        _synth((L, T, waves, 1, 0, 0, 0, 8, 0, 0, 2, 0, 0), "f32", "live8", dict(EXACT, **pin),
               f"launch_one_exact<{L}>: one-shot, `!args.live4`, neither `args.any_blend` nor"
               + (" `args.half_capable`" if L == 1 else " (L > 1) a HALF-only kernel"))
        _synth((L, T, waves, 1, 0, 1, 1, 8, 0, 0, 2, 0, 0), "f32", "odd_anybl", dict(EXACT, row_groups=0, **pin),
               f"launch_one_exact<{L}>: one-shot, `!args.live4`, `args.any_blend`")
        if L == 1:
            _synth((1, T, waves, 1, 0, 1, 0, 8, 0, 0, 2, 0, 0), "i16", "odd", dict(EXACT, row_groups=0, **pin),
                   "launch_one_exact<1>: one-shot, `!args.live4`, `!args.any_blend`, `if constexpr (L == 1)` `args.half_capable`")
        # -- exact, two waves per SIMD
        two = dict(EXACT, **pin, **TWO_WAVES)
        if L in (2, 4):
            for anybl in (0, 1):
                _synth((L, 64, waves, 2, 0, 0, anybl, 4, 0, 0, 2, 0, 0), "i16" if anybl else "f32", four[anybl], two,
                       f"launch_one_exact<{L}>: `args.cohabit && !args.state` (L = 4, or `args.live4`) -> MINW = 2; `args.live4`, "
                       f"`args.any_blend` {'set' if anybl else 'clear'}")
        if L == 4:
            _synth((4, T, waves, 2, 0, 0, 0, 8, 0, 0, 2, 0, 0), "f32", "live8", two,
                   "launch_one_exact<4>: `args.cohabit` -> MINW = 2; `!args.live4`, `!args.any_blend`")
            _synth((4, T, waves, 2, 0, 1, 1, 8, 0, 0, 2, 0, 0), "f32", "odd_anybl", dict(two, row_groups=0),
                   "launch_one_exact<4>: `args.cohabit` -> MINW = 2; `!args.live4`, `args.any_blend`")
        # -- exact, resumable
        if L <= 4:
            for anybl in (0, 1):
                _synth((L, T, waves, 1, 1, 0, anybl, 4, 0, 0, 2, 0, 0), "batch-stream", four[anybl], dict(EXACT, **pin),
                       f"launch_one_exact<{L}>: `args.state && args.live4`, `args.any_blend` {'set' if anybl else 'clear'}")
        _synth((L, T, waves, 1, 1, 0, 0, 8, 0, 0, 2, 0, 0), "batch-stream", "live8", dict(EXACT, **pin),
               f"launch_one_exact<{L}>: `args.state`, `!args.live4 && !args.any_blend && !args.half_capable`")
        if L in (1, 4):
            _synth((L, T, waves, 1, 1, 1, 1, 8, 0, 0, 2, 0, 0), "live-stream", "lean4", dict(EXACT, **pin),
                   f"launch_one_exact<{L}>: `args.state`, `!args.live4`, `args.any_blend` or `args.half_capable` (a live stream sets any_blend)")
        else:
            _synth((L, T, waves, 1, 1, 1, 1, 8, 0, 0, 2, 0, 0), "batch-stream", "odd", dict(EXACT, **pin),
                   f"launch_one_exact<{L}>: `args.state`, `!args.live4`, `args.any_blend` or `args.half_capable` (half_capable)")
        # -- tolerance, one-shot (launch_one_fast)
        fast = dict(FAST, **pin)
        TF = 64 if L == 1 else T
        if L <= 4:
            for anybl in (0, 1):
                _synth((L, 64 if L in (1, 4) else T, waves, 1, 0, 0, anybl, 4, 0, 1, 2, 0, 0), "f32", four[anybl], fast,
                       f"launch_one_fast<{L}>: `!args.state && args.live4`, `args.any_blend` {'set' if anybl else 'clear'}"
                       + (" (TF = 64)" if L == 1 else " (T4 = 64)" if L == 4 else ""))
        for anybl in (0, 1):
            _synth((L, TF, waves, 1, 0, 0, anybl, 8, 0, 1, 2, 0, 0), "f32", eight[anybl], fast,
                   f"launch_one_fast<{L}>: `!args.state`, `!args.live4`, `args.any_blend` {'set' if anybl else 'clear'}"
                   + (" (TF = 64)" if L == 1 else ""))
        # -- tolerance, two waves per SIMD
        two = dict(fast, **TWO_WAVES)
        if L in (2, 4):
            for anybl in (0, 1):
                _synth((L, 64, waves, 2, 0, 0, anybl, 4, 0, 1, 2, 0, 0), "f32", four[anybl], two,
                       f"launch_one_fast<{L}>: `args.cohabit && !args.state` (L > 2, or `args.live4`) -> MINW = 2; `args.live4`, "
                       f"`args.any_blend` {'set' if anybl else 'clear'}")
        if L in (4, 8):
            for anybl in (0, 1):
                _synth((L, T, waves, 2, 0, 0, anybl, 8, 0, 1, 2, 0, 0), "f32", eight[anybl], two,
                       f"launch_one_fast<{L}>: `args.cohabit` -> MINW = 2; `!args.live4`, `args.any_blend` {'set' if anybl else 'clear'}")
        # -- tolerance, resumable
        fast_stream = {"arithmetic": 1, **pin}
        if L <= 4:
            for anybl in (0, 1):
                _synth((L, T, waves, 1, 1, 0, anybl, 4, 0, 1, 2, 0, 0), "batch-stream", four[anybl], fast_stream,
                       f"launch_one_fast<{L}>: `args.state && args.live4`, `args.any_blend` {'set' if anybl else 'clear'}")
        _synth((L, T, waves, 1, 1, 0, 1, 8, 0, 1, 2, 0, 0), "batch-stream", "live8", fast_stream,
               f"launch_one_fast<{L}>: `args.state`, `!args.live4` (one instantiation for every blend length)")


def _one_lane_tier_entries():
    """The time-split kernels, the second tolerance tier (MID) and its time-split form: one lane per utterance."""
    corpora = {(4, 0): "lean4", (4, 1): "lean4_anybl", (8, 0): "live8", (8, 1): "live8_anybl"}
    for (nfa, anybl), name in corpora.items():
        which = f"`args.live4` {'set' if nfa == 4 else 'clear'}, `args.any_blend` {'set' if anybl else 'clear'}"
        _synth((1, 64, 1, 1, 0, 0, anybl, nfa, 0, 1, 2, 1, 0), "f32", name, dict(SPLIT, arithmetic=1),
               f"synth_kernels.hip launch_synth: `args.split_chunks`, `args.fast == 1` -> synth_inst_split.hip launch_split: {which}")
        _synth((1, 64, 1, 1, 0, 0, anybl, nfa, 0, 1, 2, 0, 1), "f32", name, {"arithmetic": 2, "lanes_per_utterance": 1},
               f"launch_synth: `args.fast == 2`, L = 1 -> synth_inst_mid.hip launch_mid_l1: `!args.state`, {which}")
        _synth((1, 64, 1, 1, 0, 0, anybl, nfa, 0, 1, 2, 1, 1), "f32", name, dict(SPLIT, arithmetic=2),
               f"launch_synth: `args.split_chunks`, `args.fast == 2` -> synth_inst_split_mid.hip launch_split_mid: {which}")
    mid_stream = {"arithmetic": 2, "lanes_per_utterance": 1}
    _synth((1, 32, 1, 1, 1, 0, 0, 4, 0, 1, 2, 0, 1), "batch-stream", "lean4", mid_stream,
           "launch_mid_l1: `args.state`, `args.live4`, `!args.any_blend`")
    _synth((1, 32, 1, 1, 1, 0, 1, 4, 0, 1, 2, 0, 1), "batch-stream", "lean4_anybl", mid_stream,
           "launch_mid_l1: `args.state`, `args.live4 && args.any_blend`")
    _synth((1, 32, 1, 1, 1, 0, 1, 8, 0, 1, 2, 0, 1), "batch-stream", "live8", mid_stream,
           "launch_mid_l1: `args.state`, `!args.live4`")


def _pipe_entries():
    """The pipelined four-wave workgroups (synth_inst_pipe.hip): exact arithmetic, small batches, no pinned mapping."""
    for L, nfa, plain, anybl in ((4, 4, "lean4", "lean4_anybl"), (8, 8, "live8", "live8_anybl")):
        for pqp, r32 in ((8, 2), (4, 0)):
            opts = dict(EXACT, lanes_per_utterance=0, ragged_plan=0, pipeline_round32=r32)
            kind = f"`args.pipe == 2` (\"pipeline_round32\" = 2)" if pqp == 8 else "`args.pipe == 1` (\"pipeline_round32\" = 0)"
            fn = f"launch_pipe{4 if L == 4 else 8} (family_choice.cpp lane_family: want_pipe{4 if L == 4 else 8})"
            # (one-shot: every slot of a workgroup taken — see pipe_fill; a resumable launch fills them whatever the option)
            full = dict(opts, pipeline_spread=0)
            _synth((L, 64, 4, 1, 0, 0, 0, nfa, 1, 0, pqp, 0, 0), "i16" if pqp == 4 else "f32", plain, full,
                   f"{fn}: `!args.state`, `!args.any_blend`, {kind}")
            _synth((L, 64, 4, 1, 0, 0, 1, nfa, 1, 0, pqp, 0, 0), "f32", anybl, full, f"{fn}: `!args.state`, `args.any_blend`, {kind}")
            _synth((L, 64, 4, 1, 1, 0, 1, nfa, 1, 0, pqp, 0, 0), "batch-stream", plain, opts,
                   f"launch_pipe{4 if L == 4 else 8} (streams.cpp stream_next: a.pipe): `args.state`, {kind}")


def _scan_entries():
    for pairs, name in ((2, "lean4"), (4, "live8")):
        for split in (1, 0):
            opts = {"arithmetic": 1, "time_split": 0}
            if not split:
                opts["time_parallel_scan_split_max_utterances"] = 0
            ENTRIES.append(Entry(scan_name((pairs, split)), "f32", name, opts, SCAN_ROWS, ONE_SHOT, "tolerance",
                                 f"family_choice.cpp scan_candidate -> scan_kernels.hip launch_scan: `args.live4` "
                                 f"{'set' if pairs == 2 else 'clear'}, `args.pipe` (scan_pipe: rows within "
                                 f"\"time_parallel_scan_split_max_utterances\") {'set' if split else 'clear'}"))


_lane_entries()
_one_lane_tier_entries()
_pipe_entries()
_scan_entries()
BY_NAME = {e.name: e for e in ENTRIES}
assert len(BY_NAME) == len(ENTRIES), [n for n, k in collections.Counter(e.name for e in ENTRIES).items() if k > 1]


def cell_id(e):
    return e.name.replace("synth_kernel<", "synth<").replace("scan_kernel<", "scan<")


def markdown():
    """The body of tests/SYNTH_KERNELS.md: one table line per entry."""
    lines = ["| kernel | routed there by | cell |", "|---|---|---|"]
    for e in sorted(ENTRIES, key=lambda e: e.name):
        opts = ", ".join(f'"{k}" = {v}' for k, v in e.options.items())
        how = ("strides " + ", ".join(str(s) for s in e.launches)) if "stream" not in e.form else \
            ("pulls of " + ", ".join(str(q) for q in e.launches) + f", then {REST}")
        form = "f32 and i16" if e.form == "i16" else e.form
        lines.append(f"| `{e.name}` | {e.route} | {form}, `{e.corpus}`[{e.rows}], {opts}; {how}; {e.arithmetic} |")
    return "\n".join(lines) + "\n"
