"""No kernel family stores outside its rows' samples.  include/grail_hip.h promises that grail_batch_synthesize_async (and
its _pcm16 and _elems forms) writes utterance u at out_dev + u * out_stride and leaves the samples past its end untouched, that
grail_stream_next_async writes each row's next samples from index 0 and the count to out_len_dev[u], and that the one-call
GRAIL_OUT_HOST forms overwrite all n_utt * out_stride floats with each row's samples followed by zeros.  Every cell below
pins one kernel family with options, asserts from grail_last_kernel_name and the read-only options that this family ran,
and renders the small ragged corpus of tests/footprint.py into a buffer with canary words around every row: behind each
row's count up to its stride, GUARD rows in front of the first row and behind the last, the bytes in front of a shifted base,
and 64 words on either side of out_len.  The rows themselves are held to the oracle (exact arithmetic: bit for bit; tolerance
arithmetic: the project's tolerance, i16 rows the conversion of the f32 rows of the same launch options).

Cells the library has no kernel for are left out, each with the reason beside the table it would stand in:
  * exact lane kernels for two waves per SIMD exist for two lanes with four formants laid out and for four lanes
    (family_cost.cpp family_cohabits): none for eight lanes, none for two lanes with eight formants;
  * the second tolerance tier has one-lane kernels only ("arithmetic" = 2 on a pinned wider mapping runs the exact kernels);
  * the time-split grid needs 512 samples of span per chunk and the span is capped at out_stride: capacities of 1021 and
    1024 give no grid of two chunks, and the pipelined exact workgroups run; a capacity can never equal a bound of its own
    grid (bounds lie inside the span), so the capacity "on a seam" is a bound of the uncut launch's grid, which cuts the
    rows inside a chunk of its own grid;
  * a composite launch at a capacity of 1021: rows that short are one launch to the planner;
  * the scan and time-split kernels take only rows the lean families take: no `odd` corpus for them.

The corpus-properties test at the top needs no GPU."""
import re

import numpy as np
import pytest

import footprint as F
import grail_hip as G
from grail_hip import workload as W

# class: (i16 rows, stride ("S": the corpus' own, nothing cut, every row a tail), base offset in samples)
CLASSES = {"a": (False, "S", 0), "b": (False, "S+1", 0), "c": (False, 1021, 0), "d": (True, "S", 0), "e": (True, "S+1", 0),
           "f": (False, "S", 1), "g": (True, "S", 1), "h": (False, 1024, 0), "i": (False, 61, 0),
           "s": (False, "seam", 0)}     # (time-split cells only: a chunk bound of the uncut launch's grid)


# ---- the corpus, from the oracle alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", F.VARIANTS)
def test_the_corpus_has_the_rows_the_cells_rely_on(variant):
    voices, segs, offs, vids, seeds, ref, ref_len, S = F.corpus(variant)
    lens = ref_len.astype(np.int64)
    assert len(lens) == F.N_UTT == 200 and len(voices) == (8 if variant == "live8" else 1)
    assert set((lens % 4).tolist()) == {0, 1, 2, 3}
    assert np.any((lens % 32 == 0) & (lens > 0))
    assert 6000 <= lens.max() < 8000
    assert S % 64 == 0 and lens.max() < S <= lens.max() + 64
    for cap in F.CAPACITIES:
        assert (lens > cap).sum() >= 20 and (lens <= cap).sum() >= 4, (cap, int((lens > cap).sum()), int((lens <= cap).sum()))
    n_segs = np.diff(offs.astype(np.int64))
    pow2 = np.log2(segs["blend_length"].astype(np.float64)) % 1 == 0
    if variant == "odd":
        assert n_segs.min() == 0 and all(np.any(lens == k) for k in (0, 1, 2, 3))
        assert np.any(segs["length"] == 0.0) and {G.PH_STOP, G.PH_GLIDE} <= set(segs["phoneme"].tolist())
    else:
        # what the four-formant, pipelined, scan and time-split families accept
        assert n_segs.min() >= 1 and segs["length"].min() * F.RATE >= 2.0
        assert set(segs["phoneme"].tolist()) <= {G.PH_A, G.PH_E, G.PH_SILENCE}
    assert pow2.all() == (variant != "lean4_anybl") and (variant != "lean4_anybl" or not pow2.any())
    assert np.isfinite(ref).all()
    # the subsets some cells take: rows that differ in length, cut and uncut ones among them
    for n in (24, 40):
        assert len(set(lens[:n].tolist())) > n // 2 and (lens[:n] > 1024).sum() >= 4 and (lens[:n] <= 61).sum() >= 1


# ---- one launch into a guarded buffer ----------------------------------------------------------------------------------
def kernel_facts(name):
    """('synth', L, T, W, MINW, {flags}) or ('scan', name)."""
    m = re.fullmatch(r"synth_kernel<L=(\d+),T=(\d+),W=(\d+),(\d+),(.*)>", name)
    if not m:
        assert name.startswith("scan_kernel<"), name
        return ("scan", name)
    return ("synth",) + tuple(int(x) for x in m.groups()[:4]) + (set(m.group(5).split(",")),)


def assert_family(ctx, want, what):
    """want: name= (the whole name), L=, T=, minw=, has= / hasnt= (flags of the name), ro= {read-only option: predicate}."""
    name = ctx.last_kernel_name()
    facts = kernel_facts(name)
    if "name" in want:
        assert name == want["name"], f"{what}: {name} ran, not {want['name']}"
    else:
        assert facts[0] == "synth", f"{what}: {name} ran"
        _, L, T, _, minw, flags = facts
        for key, got in (("L", L), ("T", T), ("minw", minw)):
            assert key not in want or want[key] == got, f"{what}: {name} ran, {key} = {want[key]} was pinned"
        missing, extra = set(want.get("has", ())) - flags, set(want.get("hasnt", ())) & flags
        assert not missing and not extra, f"{what}: {name} ran (lacks {sorted(missing)}, has {sorted(extra)})"
    for opt, pred in want.get("ro", {}).items():
        assert pred(ctx.get_option(opt)), f"{what}: {name} ran with {opt} = {ctx.get_option(opt)}"
    return name


def launch_guarded(ctx, launch, n_utt, stride, pcm16, base, counts, cut, want, what):
    """One launch into a guarded buffer; the family, the status of the sync, out_len and every canary asserted.
    Returns (the batch's own rows as uint32 / uint16 [n_utt, stride], the kernel's name)."""
    with F.Guarded(ctx, n_utt, stride, pcm16, base * (2 if pcm16 else 4)) as buf:
        launch(buf.out, stride, buf.out_len)
        status = G.OK
        try:
            ctx.sync()
        except G.GrailError as e:
            status = e.status
        name = assert_family(ctx, want, what)
        what = f"{what} ({name})"
        assert status == (G.ERR_BUFFER_TOO_SMALL if cut else G.OK), f"{what}: sync returned {status}, rows cut: {cut}"
        front, rows, lens = buf.download()
    F.check_lengths(lens, counts, what)
    F.check_guards(front, rows, lens, n_utt, counts, pcm16, what)
    return rows[F.GUARD:F.GUARD + n_utt], name


def _seam_capacity(ctx, voices, S, live8):
    """A chunk bound of the three-chunk grid of the uncut launch (span: the stride S, the longest row rounds up to it)."""
    warmup = max(G.time_split_warmup(v) for v in voices)
    bounds = G.time_split_grid(S, warmup, 3, ctx.get_option("time_split_ff_cost_permille") * (4 if live8 else 5) // 5)
    assert 0 < bounds[1] < bounds[2] < S, bounds
    return bounds[2]


def run_cell(ctx, corpus, opts, want, classes, exact=True, rows=None, repeat=1, elems=False):
    c = F.first_rows(F.corpus(corpus, repeat), rows)
    voices, segs, offs, vids, seeds, ref, ref_len, S = c
    n_utt = len(ref_len)
    saved = {k: ctx.get_option(k) for k in opts}
    ctx.set_voices(voices)
    batch = None
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        if elems:
            arr, ref, ref_len = F.sequence_oracle(c)
            batch = ctx.upload_elems(list(arr), offs, vids, seeds)
        else:
            batch = ctx.upload(segs, offs, vids, seeds)
        f32_rows = {}                           # tolerance arithmetic: stride -> the f32 rows, what the i16 rows convert
        ref_bits, ref16 = ref.view(np.uint32), None
        for label in classes:
            pcm16, stride, base = CLASSES[label]
            stride = {"S": S, "S+1": S + 1, "seam": None}.get(stride, stride)
            if stride is None:
                stride = _seam_capacity(ctx, voices, S, corpus == "live8")
            counts = np.minimum(ref_len, stride).astype(np.uint32)
            cut = bool(np.any(ref_len > stride))
            what = f"{corpus}[{n_utt}] {opts} class {label}: {'i16' if pcm16 else 'f32'} stride {stride} base +{base}"
            if pcm16 and not exact and stride not in f32_rows:
                f32_rows[stride], _ = launch_guarded(ctx, batch.synthesize_async, n_utt, stride, False, 0, counts, cut, want,
                                                     what + " (its f32 rows)")
            own, name = launch_guarded(ctx, batch.synthesize_pcm16_async if pcm16 else batch.synthesize_async, n_utt, stride,
                                       pcm16, base, counts, cut, want, what)
            what = f"{what} ({name})"
            print(what)
            if exact and pcm16:
                ref16 = F.pcm16_of(ref).view(np.uint16) if ref16 is None else ref16
                F.check_bits(own, ref16, counts, what)
            elif exact:
                F.check_bits(own, ref_bits, counts, what)
            elif pcm16:
                F.check_tolerance(f32_rows[stride], ref, counts, what + " (its f32 rows)")
                F.check_bits(own, F.pcm16_of(f32_rows[stride].view(np.float32)).view(np.uint16), counts, what)
            else:
                worst = F.check_tolerance(own, ref, counts, what)
                print(f"    worst {worst / 2.0 ** -23:.1f} * 2^-23 of max(1, peak)")
                if base == 0:
                    f32_rows.setdefault(stride, own)
    finally:
        if batch is not None:
            batch.free()
        for k, v in saved.items():
            ctx.set_option(k, v)
        ctx.set_voices(W.single_voice())


def _cells():
    cells = []

    def cell(name, corpus, opts, want, classes, **kw):
        cells.append(pytest.param(corpus, opts, want, classes, kw, id=f"{name}-{corpus}"))

    exact = {"hasnt": ("FAST", "PIPE", "STREAM", "SPLIT", "MID")}
    # -- exact arithmetic ----------------------------------------------------------------------------------------------
    # lane kernels with four formants laid out, both ways of dividing alpha out (eight lanes lay out eight formants
    # whatever the voices: family_choice.cpp choose_family)
    for L in (2, 4, 8):
        for corpus, any_blend in (("lean4", False), ("lean4_anybl", True)):
            w = dict(exact, L=L, has=("NFA=4" if L < 8 else "NFA=8",) + (("ANYBL",) if any_blend else ()))
            w["hasnt"] = exact["hasnt"] + (() if any_blend else ("ANYBL",))
            cell(f"exact-L{L}", corpus, {"lanes_per_utterance": L}, w, "abcde" + ("fg" if L in (2, 8) else ""))
    cell("exact-L1", "lean4_anybl", {"lanes_per_utterance": 1}, dict(exact, L=1, has=("NFA=4", "ANYBL")), "abcdefg")
    for L in (1, 2, 4, 8):
        cell(f"exact-L{L}", "live8", {"lanes_per_utterance": L}, dict(exact, L=L, has=("NFA=8",), hasnt=exact["hasnt"] + ("ANYBL",)),
             "abcde")
        # the general instantiations: rows without segments, of 1 - 3 samples, zero-length segments, Stop and Glide
        # ("row_groups" = 0: every row of the batch on them, none planned apart)
        cell(f"general-L{L}", "odd", {"lanes_per_utterance": L, "row_groups": 0}, dict(exact, L=L, has=("NFA=8",)), "abdhi")
    # rows planned apart: the odd rows in a launch of their own
    for L in (0, 1, 4):
        cell(f"row-groups-L{L}", "odd", {"row_groups": 2, "lanes_per_utterance": L},
             {"hasnt": ("FAST", "STREAM", "SPLIT", "MID"), "ro": {"last_launch_blocks": lambda v: v >= 2}}, "ad")
    # pipelined workgroups in rounds of 32 and of 16 samples (the four-wave share of the flush)
    for r32, flag in ((2, "R32"), (0, "R16")):
        for corpus in ("lean4", "live8", "lean4_anybl"):
            cell(f"pipe-{flag}", corpus, {"lanes_per_utterance": 0, "ragged_plan": 0, "pipeline_round32": r32},
                 {"has": ("PIPE", flag, "NFA=8" if corpus == "live8" else "NFA=4"), "hasnt": ("FAST", "STREAM"),
                  "ro": {"last_launch_pipelined": lambda v: v >= 1}}, "abcdeh")
    for spread in (1, 0):
        cell(f"pipe-spread{spread}", "lean4", {"lanes_per_utterance": 0, "ragged_plan": 0, "pipeline_spread": spread},
             {"has": ("PIPE", "NFA=4"), "hasnt": ("FAST", "STREAM")}, "ad", rows=40)
    # two waves per SIMD (the fourth number of the name) on a device assumed to have four SIMDs
    for two in (1, 0):
        for L, corpus in ((2, "lean4"), (4, "lean4"), (4, "live8")):
            cell(f"two-waves{two}-L{L}", corpus, {"assume_compute_units": 1, "lanes_per_utterance": L, "two_waves_per_simd": two},
                 dict(exact, L=L, minw=2 if two else 1), "abd")
    # packed launch order: eleven one-wave workgroups of rows that differ in length on four SIMDs (704 rows: where the
    # library's dispatch model gains 3 % by packing; it takes a packed order from 1.5 %)
    for packed in (1, 0):
        cell(f"packed{packed}", "lean4", {"assume_compute_units": 1, "lanes_per_utterance": 1, "packed_launch_order": packed},
             dict(exact, L=1, ro={"last_launch_packed": (lambda v: v >= 1) if packed else (lambda v: v == 0)}), "ad", repeat=4, rows=704)
    # composite launch: a batch cut into blocks by size, each block its own family (out_shift).  (No capacity of 1021: rows
    # that short are one launch to the planner, which is no composite launch.)
    cell("composite", "lean4", {"assume_compute_units": 1, "ragged_plan": 0},
         {"hasnt": ("FAST", "STREAM"), "ro": {"last_launch_blocks": lambda v: v >= 2}}, "abd", repeat=2)
    # the caller's order and the length-sorted slots (rows looked up through the permutation)
    for sort in (0, 1):
        for L in (1, 4):
            cell(f"sort{sort}-L{L}", "lean4", {"sort_by_length": sort, "lanes_per_utterance": L}, dict(exact, L=L, has=("NFA=4",)), "a")
    # caller-built elems
    cell("elems-L0", "lean4", {"lanes_per_utterance": 0}, {"has": ("NFA=4",), "hasnt": ("FAST", "STREAM")}, "ad", elems=True)
    cell("elems-L2", "lean4", {"lanes_per_utterance": 2}, dict(exact, L=2, has=("NFA=4",)), "ad", elems=True)
    # -- tolerance arithmetic --------------------------------------------------------------------------------------------
    fast = {"arithmetic": 1, "time_split": 0, "time_parallel_scan": 0}
    for L in (1, 2, 4, 8):
        for corpus in ("lean4", "live8"):
            w = {"L": L, "has": ("FAST",), "hasnt": ("PIPE", "STREAM", "SPLIT", "MID"), "ro": {"last_launch_fast": lambda v: v == 1}}
            if L == 1:
                w["T"] = 64         # the row-step flush
            cell(f"fast-L{L}", corpus, dict(fast, lanes_per_utterance=L), w, "abcdehi" + ("fg" if L == 1 else ""), exact=False)
    cell("mid-L1", "lean4", {"arithmetic": 2, "lanes_per_utterance": 1},
         {"L": 1, "has": ("FAST", "MID"), "hasnt": ("SPLIT", "PIPE", "STREAM"), "ro": {"last_launch_fast": lambda v: v == 2}}, "abd",
         exact=False)
    for corpus, pairs in (("lean4", 2), ("live8", 4)):
        for split in (1, 0):
            opts = {"arithmetic": 1, "time_split": 0}
            if not split:
                opts["time_parallel_scan_split_max_utterances"] = 0
            cell(f"scan-split{split}", corpus, opts, {"name": "scan_kernel<pairs=%d,%sFAST>" % (pairs, "SPLIT," if split else "")},
                 "abcdehi", exact=False, rows=24)
        for chunks in (3, 0):
            cell(f"time-split-chunks{chunks}", corpus,
                 {"arithmetic": 1, "time_parallel_scan": 0, "time_split_min_utterances": 0, "composite_launches": 0,
                  "time_split_chunks": chunks},
                 {"L": 1, "has": ("FAST", "SPLIT"), "hasnt": ("MID",), "ro": {"last_launch_chunks": lambda v: v >= 2}}, "abds",
                 exact=False)
    return cells


@pytest.mark.gpu
@pytest.mark.parametrize("corpus,opts,want,classes,kw", _cells())
def test_one_shot_launches_store_only_their_rows_samples(gpu_ctx, corpus, opts, want, classes, kw):
    run_cell(gpu_ctx, corpus, opts, want, classes, **kw)


# ---- streams -----------------------------------------------------------------------------------------------------------
PULLS = ((1, 512), (63, 512), (64, 512), (65, 512), (500, 512), (2000, 2001))       # (max_samples, stride), in turn


def pull_guarded(ctx, stream, q, stride, pcm16, n_utt, want, what):
    """One pull into a freshly guarded buffer.  Returns (the rows [n_utt, stride], the counts)."""
    with F.Guarded(ctx, n_utt, stride, pcm16) as buf:
        (stream.next_pcm16_async if pcm16 else stream.next_async)(q, buf.out, stride, buf.out_len)
        ctx.sync()
        what = f"{what} ({assert_family(ctx, want, what)})"
        front, rows, lens = buf.download()
    counts = lens[F.LEN_GUARD:F.LEN_GUARD + n_utt]
    assert counts.max(initial=0) <= q, f"{what}: row {int(np.argmax(counts))} got {int(counts.max())} samples of a quota of {q}"
    F.check_guards(front, rows, lens, n_utt, counts, pcm16, what)
    return rows[F.GUARD:F.GUARD + n_utt], counts.copy()


def check_concatenation(chunks, ref, ref_len, exact, what):
    """chunks[u]: [(i16?, samples as uint32 / uint16)] in order."""
    ref16 = F.pcm16_of(ref).view(np.uint16)
    worst = 0.0
    for u in range(len(ref_len)):
        n, at = int(ref_len[u]), 0
        assert sum(len(x) for _, x in chunks[u]) == n, f"{what}: row {u} yielded {sum(len(x) for _, x in chunks[u])} samples, not {n}"
        peak = max(1.0, float(np.abs(ref[u, :n]).max(initial=0.0)))
        for pcm16, x in chunks[u]:
            m = len(x)
            if exact or pcm16:          # (tolerance streams here pull f32 only)
                want = ref16[u, at:at + m] if pcm16 else ref[u, at:at + m].view(np.uint32)
                bad = np.flatnonzero(x != want)
                assert len(bad) == 0, f"{what}: row {u} sample {at + int(bad[0])} of {n} is {int(x[bad[0]]):#x}, not {int(want[bad[0]]):#x}"
            else:
                d = np.abs(x.view(np.float32).astype(np.float64) - ref[u, at:at + m])
                assert np.all(d <= G.FAST_TOLERANCE * peak), f"{what}: row {u} sample {at + int(np.argmax(d))} of {n} is off by {d.max() / 2.0 ** -23:.1f} * 2^-23"
                worst = max(worst, float(d.max(initial=0.0)) / peak)
            at += m
    return worst


def _stream_family(lanes, fast=False):
    if lanes == 0:      # small batches: the pipelined workgroups, in exact arithmetic whatever was asked for
        return {"has": ("STREAM", "PIPE"), "hasnt": ("FAST",)}
    return {"L": lanes, "has": ("STREAM",) + (("FAST",) if fast else ()), "hasnt": ("PIPE",) + (() if fast else ("FAST",))}


@pytest.mark.gpu
@pytest.mark.parametrize("corpus,lanes,fast", [(c, L, 0) for c in ("lean4", "odd") for L in (0, 1, 2, 8)] + [("lean4", 0, 1), ("lean4", 1, 1)])
def test_batch_streams_store_only_their_chunks(gpu_ctx, corpus, lanes, fast):
    """Quotas of 1, 63, 64, 65 and 500 samples into rows of 512 and of 2000 into rows of 2001, f32 and i16 pulls in turn
    (tolerance arithmetic: f32): no pull yields more than its quota or writes past a row's count, and the chunks
    concatenate to the oracle's rows."""
    ctx = gpu_ctx
    voices, segs, offs, vids, seeds, ref, ref_len, S = F.corpus(corpus)
    n_utt = len(ref_len)
    opts = {"lanes_per_utterance": lanes, "arithmetic": fast}
    saved = {k: ctx.get_option(k) for k in opts}
    ctx.set_voices(voices)
    batch = st = None
    chunks = [[] for _ in range(n_utt)]
    try:
        for name, v in opts.items():
            ctx.set_option(name, v)
        batch = ctx.upload(segs, offs, vids, seeds)
        st = G.Stream(batch)
        names = set()
        for k in range(1000):
            q, stride = PULLS[k % len(PULLS)]
            pcm16 = bool(k % 2) and not fast
            what = f"stream of {corpus} {opts}, pull {k}: {'i16' if pcm16 else 'f32'} quota {q} stride {stride}"
            rows, counts = pull_guarded(ctx, st, q, stride, pcm16, n_utt, _stream_family(lanes, fast), what)
            names.add(ctx.last_kernel_name())
            if counts.max(initial=0) == 0:
                break
            for u in range(n_utt):
                chunks[u].append((pcm16, rows[u, :counts[u]].copy()))
        else:
            raise AssertionError("the stream never ended")
    finally:
        if st is not None:
            st.close()
        if batch is not None:
            batch.free()
        for name, v in saved.items():
            ctx.set_option(name, v)
        ctx.set_voices(W.single_voice())
    print(f"stream of {corpus} {opts}: {k + 1} pulls of {sorted(names)}")
    worst = check_concatenation(chunks, ref, ref_len, not fast, f"stream of {corpus} {opts}")
    if fast:
        print(f"    worst {worst / 2.0 ** -23:.1f} * 2^-23 of max(1, peak)")


@pytest.mark.gpu
@pytest.mark.parametrize("pcm16", [False, True])
def test_live_streams_store_only_their_chunks(gpu_ctx, pcm16):
    """Segments appended two at a time between pulls of 1 500 samples: a row whose two segments are shorter than that pauses
    inside the chunk (fewer samples than the quota for a row that is not finished), then `finish`."""
    ctx = gpu_ctx
    voices, segs, offs, vids, seeds, ref, ref_len, S = F.corpus("lean4")
    n_utt = len(ref_len)
    q, stride = 1500, 1501
    ctx.set_voices(voices)
    st = G.LiveStream(ctx, n_utt, vids, seeds, ring_segments=8)
    chunks = [[] for _ in range(n_utt)]
    fed = offs[:-1].astype(np.int64).copy()
    done = np.zeros(n_utt, dtype=np.int64)
    paused = 0
    finished = False
    want = {"has": ("STREAM",), "hasnt": ("FAST",)}
    try:
        for k in range(1000):
            if not finished:
                upto = np.minimum(fed + 2, offs[1:].astype(np.int64))
                if np.any(upto > fed):
                    st.append(np.concatenate([segs[fed[u]:upto[u]] for u in range(n_utt)]),
                              np.concatenate([[0], np.cumsum(upto - fed)]).astype(np.uint32))
                    fed = upto
                else:
                    st.finish()
                    finished = True
            rows, counts = pull_guarded(ctx, st, q, stride, pcm16, n_utt, want, f"live stream, pull {k}, {'i16' if pcm16 else 'f32'}")
            done += counts
            paused += int(((counts < q) & (done < ref_len)).sum())
            if finished and counts.max(initial=0) == 0:
                break
            for u in range(n_utt):
                chunks[u].append((pcm16, rows[u, :counts[u]].copy()))
        else:
            raise AssertionError("the live stream never ended")
    finally:
        st.close()
        ctx.set_voices(W.single_voice())
    print(f"live stream, {'i16' if pcm16 else 'f32'}: {k + 1} pulls of {ctx.last_kernel_name()}, {paused} rows paused inside a chunk")
    assert paused >= 20, paused
    check_concatenation(chunks, ref, ref_len, True, "live stream")


# ---- the one-call host forms -------------------------------------------------------------------------------------------
def _host_cells():
    cells = []
    fast = {"arithmetic": 1, "time_split": 0, "time_parallel_scan": 0}
    groups = [("L1", {"lanes_per_utterance": 1}, {"L": 1, "hasnt": ("FAST", "PIPE")}, True, None, ("lean4", "odd")),
              ("L8", {"lanes_per_utterance": 8}, {"L": 8, "hasnt": ("FAST", "PIPE")}, True, None, ("lean4", "odd")),
              ("pipe", {"lanes_per_utterance": 0, "ragged_plan": 0}, {"has": ("PIPE",), "hasnt": ("FAST",)}, True, None, ("lean4", "odd")),
              ("fast-L1", dict(fast, lanes_per_utterance=1), {"L": 1, "T": 64, "has": ("FAST",), "hasnt": ("SPLIT", "MID")}, False, None,
               ("lean4", "odd")),
              # (the scan and time-split kernels take only rows the lean families take; one chunk at a capacity of 1021)
              ("scan", {"arithmetic": 1, "time_split": 0}, {"name": "scan_kernel<pairs=2,SPLIT,FAST>"}, False, 24, ("lean4",)),
              ("time-split", {"arithmetic": 1, "time_parallel_scan": 0, "time_split_min_utterances": 0, "composite_launches": 0,
                              "time_split_chunks": 3}, {"L": 1, "has": ("FAST", "SPLIT")}, False, None, ("lean4",))]
    for name, opts, want, exact, rows, corpora in groups:
        for corpus in corpora:
            for stride in ("S", 1021):
                if name == "time-split" and stride == 1021:
                    continue
                cells.append(pytest.param(corpus, opts, want, exact, rows, stride, id=f"{name}-{corpus}-{stride}"))
    return cells


@pytest.mark.gpu
@pytest.mark.parametrize("corpus,opts,want,exact,rows,stride", _host_cells())
def test_host_forms_overwrite_every_row_with_its_samples_and_zeros(gpu_ctx, corpus, opts, want, exact, rows, stride):
    ctx = gpu_ctx
    voices, segs, offs, vids, seeds, ref, ref_len, S = F.first_rows(F.corpus(corpus), rows)
    n_utt = len(ref_len)
    stride = S if stride == "S" else stride
    counts = np.minimum(ref_len, stride).astype(np.uint32)
    cut = bool(np.any(ref_len > stride))
    out = np.full((n_utt, stride), F.CANARY, dtype=np.uint32).view(np.float32)
    out_len = np.full(n_utt, F.LEN_CANARY, dtype=np.uint32)
    saved = {k: ctx.get_option(k) for k in opts}
    what = f"host form of {corpus}[{n_utt}] {opts} stride {stride}"
    ctx.set_voices(voices)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        status = G.OK
        try:
            ctx.synthesize_into(out, out_len, segs, offs, vids, seeds)
        except G.GrailError as e:
            status = e.status
        what = f"{what} ({assert_family(ctx, want, what)})"
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)
        ctx.set_voices(W.single_voice())
    print(what)
    assert status == (G.ERR_BUFFER_TOO_SMALL if cut else G.OK), f"{what}: returned {status}, rows cut: {cut}"
    bad = np.flatnonzero(out_len != counts)
    assert len(bad) == 0, f"{what}: out_len[{bad[0]}] is {int(out_len[bad[0]])}, not {int(counts[bad[0]])}"
    own = out.view(np.uint32)
    if exact:
        F.check_bits(own, ref.view(np.uint32), counts, what)
    else:
        F.check_tolerance(own, ref, counts, what)
    past = np.arange(stride)[None, :] >= counts.astype(np.int64)[:, None]
    bad = F.first_bad(past & (own != 0))
    assert bad is None, (f"{what}: row {bad[0]} of {int(counts[bad[0]])} samples holds {int(own[bad]):#x} at index {bad[1]}, not +0.0 "
                         f"({int((past & (own != 0)).sum())} words)")
