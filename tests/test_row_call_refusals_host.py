"""What the calls that write rows (csrc/transforms.cpp: grail_limit_async, grail_resample_async, grail_fir_async;
csrc/transform_streams.cpp: grail_filter_stream_next_async, grail_filter_stream_finish_async) answer to arguments from the
edges of their checks, held against a recorded table: tests/golden/row_call_refusals.json is what the library of commit
8af9941 answered, when the four copies of the row-pair check still stood in levels.cpp and fir_plan.cpp, to the tuples that
the seeded generator below produces.  Every call passes ctx = NULL and addresses nobody looks behind, so no device is needed
and none is used: a tuple that gets past every argument check ends at the question for the device (GRAIL_ERR_NO_DEVICE on a
machine without one, "ctx is NULL" on a machine with one), and both are recorded as "past the checks".  Status and full
message must be equal tuple by tuple.

The table's second part, "streams", holds the other calls on streams to the same: the feeding and finishing calls of resample
and limit streams, and all three kinds' open and close.  It is what the library of commit 19f4b0d answered, when every kind of
stream still had its own copy of the host code in transforms.cpp, to the tuples of a second seeded generator: the first
part's draws, digest and answers are as they were recorded.

`PYTHONPATH=.:grail-rs_amd python tests/test_row_call_refusals_host.py [rows] [streams]` writes the parts named (none: both)
anew from the built library: only on a commit whose refusals are meant to change."""
import ctypes as C
import hashlib
import json
import math
import os
import struct

import grail_hip as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "row_call_refusals.json")
SEED = 0x8AF9941
STREAM_SEED = 0x19F4B0D
PER_ENTRY = 320
PAST = "past the checks"
FINE = (0, "")                   # GRAIL_OK (the message of an earlier refusal is not this call's)
M64 = (1 << 64) - 1

# ---- the edge grid ------------------------------------------------------------------------------------------------------------------
# (value, weight): the weights lean towards what a call takes, so that refusals further down the order are reached too and
# at least a quarter of an entry point's tuples get past every check
STRIDES = [(0, 2), (1, 2), (64, 6), (2 ** 32 - 1, 2), (2 ** 32, 2), (2 ** 61, 1)]
N_ROWS = [(0, 1), (1, 3), (2, 3), (1024, 3)]
OUT = [("disjoint", 8), ("abuts behind", 2), ("abuts before", 2), ("overlaps behind", 1), ("overlaps before", 1), ("null", 1)]
GROUPS = [(1, 10), (3, 1), (0, 1)]
CEILINGS = [(1.0, 12), (0.0, 1), (math.nan, 1), (math.inf, 1)]
LOOKAHEADS = [(10, 10), (11, 1)]
RATES = [((44100, 48000), 4), ((48000, 44100), 4), ((1, 2), 3), ((16000, 48000), 2), ((48000, 48000), 1), ((0, 48000), 1), ((48000, 0), 1)]
IN_BASE, LEN, HANDLE = 1 << 48, 0x30000000, 0x40000000           # addresses nobody looks behind


class Draws:
    """splitmix64, written out: the tuples must not depend on the Python version's random module"""

    def __init__(self, seed):
        self.s = seed & M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def pick(self, weighted):
        at = self.next() % sum(w for _, w in weighted)
        for value, w in weighted:
            if at < w:
                return value
            at -= w
        raise AssertionError

    def chance(self, one_in):
        return self.next() % one_in == 0


def out_address(kind, n_rows, in_stride, out_stride):
    """out relative to n_rows rows at IN_BASE, in bytes of float32 and modulo 2^64 as the addresses are"""
    in_bytes, out_bytes = n_rows * in_stride * 4, n_rows * out_stride * 4
    if kind == "null":
        return None
    at = {"disjoint": IN_BASE + in_bytes + 4096, "abuts behind": IN_BASE + in_bytes, "abuts before": IN_BASE - out_bytes,
          "overlaps behind": IN_BASE + in_bytes - 4, "overlaps before": IN_BASE - out_bytes + 4}[kind]
    return (at & M64) or None


def row_pair(d, n_rows, stream=False):
    """(in, in_stride, len, out, out_stride): mostly what a call takes, every field now and then from the edge grid"""
    in_stride = d.pick(STRIDES)
    out_stride = in_stride if d.chance(2) else d.pick(STRIDES)
    if stream and out_stride < in_stride and not d.chance(4):
        out_stride = in_stride
    out = out_address(d.pick(OUT), n_rows, in_stride, out_stride)
    return (None if d.chance(24) else IN_BASE, in_stride, None if d.chance(24) else LEN, out, out_stride)


def tuples():
    """{entry point: [argument tuple, ...]}, ctx (NULL) left out"""
    d = Draws(SEED)
    calls = {name: [] for name in ("grail_limit_async", "grail_resample_async", "grail_fir_async",
                                   "grail_filter_stream_next_async", "grail_filter_stream_finish_async")}
    for _ in range(PER_ENTRY):
        n = d.pick(N_ROWS)
        rows, stride, ln, out, out_stride = row_pair(d, n)
        calls["grail_limit_async"].append((rows, stride, ln, n, d.pick(GROUPS), d.pick(CEILINGS), d.pick(LOOKAHEADS), out, out_stride,
                                           None, None, None))
        n = d.pick(N_ROWS)
        rows, stride, ln, out, out_stride = row_pair(d, n)
        calls["grail_resample_async"].append((rows, stride, ln, n, *d.pick(RATES), out, out_stride, None, None))
        n = d.pick(N_ROWS)
        rows, stride, ln, out, out_stride = row_pair(d, n)
        calls["grail_fir_async"].append((None if d.chance(16) else HANDLE, rows, stride, ln, n, None, out, out_stride, None, None))
        # (without a context a stream's checks run for one row and a set of one tap)
        rows, stride, ln, out, out_stride = row_pair(d, 1, stream=True)
        calls["grail_filter_stream_next_async"].append((None if d.chance(16) else HANDLE, rows, stride, ln, out, out_stride, None, None))
        rows, stride, ln, out, out_stride = row_pair(d, 1)
        calls["grail_filter_stream_finish_async"].append((None if d.chance(8) else HANDLE, None, out, out_stride, None))
    return calls


def stream_tuples():
    """{entry point: [argument tuple, ...]} of the table's second part, ctx (NULL) left out"""
    d = Draws(STREAM_SEED)
    kinds = ("filter", "resample", "limit")
    calls = {f"grail_{kind}_stream_{call}": [] for kind in kinds[1:] for call in ("next_async", "finish_async")}
    calls.update({f"grail_{kind}_stream_{call}": [] for call in ("open", "close") for kind in kinds})
    some = lambda address, one_in: None if d.chance(one_in) else address
    for _ in range(PER_ENTRY):
        # (without a context a stream's checks run for one row, alone in its group: a ratio of 1 / 1 with two taps, a tail of
        # one output; a look-ahead of one sample, a delay of 11)
        for kind, results in (("resample", 2), ("limit", 4)):
            rows, stride, ln, out, out_stride = row_pair(d, 1, stream=True)
            calls[f"grail_{kind}_stream_next_async"].append((some(HANDLE, 16), rows, stride, ln, out, out_stride) + (None,) * results)
            rows, stride, ln, out, out_stride = row_pair(d, 1)
            calls[f"grail_{kind}_stream_finish_async"].append((some(HANDLE, 8), some(LEN, 2), out, out_stride) + (None,) * (results - 1))
        # (open without a context: the arguments from both sides of every check, `out` there and not)
        calls["grail_filter_stream_open"].append((some(HANDLE, 4), d.pick(N_ROWS), some(LEN, 2), some(HANDLE + 64, 4)))
        calls["grail_resample_stream_open"].append((*d.pick(RATES), d.pick(N_ROWS), some(HANDLE + 64, 4)))
        calls["grail_limit_stream_open"].append((d.pick(N_ROWS), d.pick(GROUPS), d.pick(CEILINGS), d.pick(LOOKAHEADS), some(HANDLE + 64, 4)))
        for kind in kinds:
            calls[f"grail_{kind}_stream_close"].append((some(HANDLE, 2),))
    return calls


def tuples_digest(calls):
    h = hashlib.sha256()
    for name in sorted(calls):
        for args in calls[name]:
            words = [struct.pack("<d", a).hex() if isinstance(a, float) else a for a in args]
            h.update((name + repr(words)).encode())
    return h.hexdigest()


def answers(lib, calls):
    """{entry point: [(status, message) or PAST, ...]}"""
    got = {}
    for name, argument_tuples in calls.items():
        fn, got[name] = getattr(lib, name), []
        for args in argument_tuples:
            status = fn(None, *args)
            message = lib.grail_last_error().decode()
            past = status == G.ERR_NO_DEVICE or (status == G.ERR_INVALID_ARG and message == name + ": ctx is NULL")
            got[name].append(PAST if past else FINE if status == G.OK else (status, message))
    return got


# Every refusal that a call with ctx = NULL can get from transforms.cpp, transform_streams.cpp, row_checks.h and the stream checks of the three plan files.
# Not reachable without a context, and so not in the table: "not a filter set / not an open filter stream of this context"
# (nothing is looked up), "more than 2^31 chunks" of the limiter and the resampler (said after the device is asked for) and
# of a stream call (one row has at most 2^21 chunks), the FIR call's "2^32 output samples" (a tail of 0 adds nothing to a
# row of fewer than 2^32 samples), and what finish says about out (a set of one tap has no tail to write).
REACHABLE = {
    "grail_limit_async": ["lookahead_log2 is above 10", "n_rows is no multiple of group", "the ceiling is not a finite number above 0",
                          "out_stride < row_stride", "NULL buffer", "the rows span more than 2^60 samples",
                          "out_dev overlaps rows_dev (the look-ahead reads ahead of the stores)"],
    "grail_resample_async": ["the rates are equal, 0, or need more than 32 768 table entries", "NULL buffer",
                             "the rows span more than 2^60 samples", "out_dev overlaps rows_dev (a chunk reads what another would have written)",
                             "a row could hold 2^32 output samples or more (out_len is 32 bits wide)"],
    "grail_fir_async": ["set is NULL", "NULL buffer", "the rows span more than 2^60 samples",
                        "out_dev overlaps rows_dev (a chunk reads what another would have written)", "more than 2^31 chunks"],
    "grail_filter_stream_next_async": ["the stream is NULL", "out_stride < in_stride (a stream never cuts outputs short)", "NULL buffer",
                                       "the rows span more than 2^60 samples",
                                       "out_dev overlaps in_dev (a chunk reads what another would have written)"],
    "grail_filter_stream_finish_async": ["the stream is NULL"],
    # (the second part.  One row at 1 / 1 has a tail of one output and one row alone a delay of 11, so these two finishing
    # calls do look at out; "more than 2^31 chunks" stays out of reach as above)
    "grail_resample_stream_next_async": ["the stream is NULL", "out_stride < ceil(in_stride * up / down) (a stream never cuts outputs short)",
                                         "NULL buffer", "the rows span more than 2^60 samples",
                                         "out_dev overlaps in_dev (a chunk reads what another would have written)"],
    "grail_resample_stream_finish_async": ["the stream is NULL", "out_stride < ceil((taps / 2) * up / down), the longest tail",
                                           "NULL buffer", "the rows span more than 2^60 samples"],
    "grail_limit_stream_next_async": ["the stream is NULL", "out_stride < in_stride (a stream never cuts outputs short)", "NULL buffer",
                                      "the rows span more than 2^60 samples",
                                      "out_dev overlaps in_dev (a chunk reads what another would have written)"],
    "grail_limit_stream_finish_async": ["the stream is NULL",
                                        "out_stride is below the stream's delay, GRAIL_LIMIT_STREAM_DELAY(lookahead_log2)",
                                        "NULL buffer", "the rows span more than 2^60 samples"],
}

# What open and close can answer without a context, in full: two opens say "NULL argument" before they look at anything, the
# limit stream's says what is wrong with its numbers first; a close of no stream is fine, and one of a stream asks for the
# context ("ctx is NULL": recorded as past the checks).
OPEN_CLOSE = {
    "grail_filter_stream_open": ["NULL argument"],
    "grail_resample_stream_open": ["NULL argument"],
    "grail_limit_stream_open": ["lookahead_log2 is above 10", "n_rows is no multiple of group", "the ceiling is not a finite number above 0",
                                "n_rows is 0", "NULL argument"],
    "grail_filter_stream_close": [FINE, PAST],
    "grail_resample_stream_close": [FINE, PAST],
    "grail_limit_stream_close": [FINE, PAST],
}


def check_coverage(got):
    for name, rows in got.items():
        assert len(rows) == PER_ENTRY, name
        if name in OPEN_CLOSE:
            want = {a if isinstance(a, tuple) or a == PAST else (G.ERR_INVALID_ARG, name + ": " + a) for a in OPEN_CLOSE[name]}
            assert set(rows) == want, (name, sorted(map(str, set(rows))))
            print(f"{name}: {len(want)} distinct answers")
            continue
        said = {a[1] for a in rows if a != PAST}
        assert all(a[0] == G.ERR_INVALID_ARG for a in rows if a != PAST), name
        assert said == {name + ": " + text for text in REACHABLE[name]}, (name, sorted(said))
        past = sum(a == PAST for a in rows)
        print(f"{name}: {past} of {len(rows)} past the checks, {len(said)} distinct refusals")
        assert len(rows) == PER_ENTRY and 4 * past >= len(rows), (name, past)


def held_to(table, calls):
    assert tuples_digest(calls) == table["tuples_sha256"], "the generator no longer produces the tuples that were recorded"
    messages = [PAST if m == PAST else tuple(m) for m in table["messages"]]
    want = {name: [messages[i] for i in table["answers"][name]] for name in calls}
    check_coverage(want)
    got = answers(G.load(), calls)
    for name in calls:
        for args, g, w in zip(calls[name], got[name], want[name]):
            assert g == w, (name, args)


def test_every_call_answers_as_recorded(built):
    with open(TABLE) as f:
        held_to(json.load(f), tuples())


def test_every_stream_call_answers_as_recorded(built):
    with open(TABLE) as f:
        held_to(json.load(f)["streams"], stream_tuples())


def recorded(seed, calls, commit):
    got = answers(G.load(), calls)
    check_coverage(got)
    messages = [PAST] + sorted({a for rows in got.values() for a in rows if a != PAST})
    return {"recorded_at": commit, "seed": seed, "tuples_sha256": tuples_digest(calls), "messages": messages,
            "answers": {name: [messages.index(a) for a in rows] for name, rows in got.items()}}


if __name__ == "__main__":
    import subprocess
    import sys

    import __graft_entry__ as ge
    ge.build()
    parts = sys.argv[1:] or ["rows", "streams"]
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    with open(TABLE) as f:
        table = json.load(f)
    streams = table.pop("streams", None)
    if "rows" in parts:
        table = recorded(SEED, tuples(), commit)
    table["streams"] = recorded(STREAM_SEED, stream_tuples(), commit) if "streams" in parts else streams
    with open(TABLE, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(f"{TABLE}: {os.path.getsize(TABLE)} bytes at {commit}")
