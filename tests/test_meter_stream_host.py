"""Meter streams without a device: the numpy model of tests/meter_stream_model.py against the one-shot models over the splits
that can go wrong (every clause of the header's contract, "levels, continued: the meters on streams"); grail_meter_stream_hops
against integer arithmetic; every refusal the calls can give with ctx = NULL, in the manner of
tests/test_row_call_refusals_host.py (addresses nobody looks behind; a call that gets past its checks ends at the question for
the device); and the library exports what the header declares."""
import ctypes as C
import re

import numpy as np
import pytest

import grail_hip as G
from meter_stream_model import (REFUSED, RowModel, bits, check_against_one_shot, hops_of_call, random_split, same_read,
                                stream_model)
from test_loudness_host import kweighting_model

RATE = 2560                     # H = 256, the smallest hop: at this rate the filter forgets only 0.28 a hop
H = RATE // 10
COEF = kweighting_model(48000)  # (what the segmented GPU tests do: a state one bit off shows in every later hop)
IN, LEN, HANDLE, OUT = 1 << 48, 0x30000000, 0x40000000, 1 << 50        # addresses nobody looks behind
PAST = "past the checks"


def noise(n, seed, amplitude=0.5):
    return np.random.default_rng(seed).uniform(-amplitude, amplitude, n).astype(np.float32)


# ---- the model against the one-shot models ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_splits(seed):
    rng = np.random.default_rng(900 + seed)
    x = noise(6 * H + 77, seed)
    x[[0, 5 * H, len(x) - 1]] = [np.nan, np.inf, -np.inf]
    for _ in range(3):
        check_against_one_shot(x, random_split(len(x), rng), RATE, COEF)
    check_against_one_shot(x, [len(x)], RATE, COEF)


def test_splits_of_one_sample():
    x = noise(2 * H + 3, 11)
    x[[H - 1, H]] = [np.nan, np.inf]
    calls, _, _, _ = check_against_one_shot(x, [1] * len(x), RATE, COEF)
    assert [len(c[0]) for c in calls].count(1) == 2 and sum(c[2] for c in calls) == 2


def test_splits_that_end_exactly_on_hop_ends():
    x = noise(5 * H, 12)
    calls, reads, _, last = check_against_one_shot(x, [H, 0, 2 * H, H, H], RATE, COEF)
    assert [len(c[0]) for c in calls] == [1, 0, 2, 1, 1] and [r[4] for r in reads] == [1, 1, 3, 4, 5] and last[0] > 0
    check_against_one_shot(x, [H - 1, 1, H + 1, H - 1, 2 * H], RATE, COEF)


def test_calls_of_zeros_and_of_nothing():
    x = np.concatenate([noise(2 * H, 13), np.zeros(3 * H, np.float32), noise(H + 5, 14)])
    calls, _, _, _ = check_against_one_shot(x, [2 * H, 0, H, 0, 0, 2 * H, H + 5, 0], RATE, COEF)
    # the filter rings on through fed zeros: their hops are not +0.0
    assert all(v > 0 for v in calls[2][0]) and calls[2][1] > 0


@pytest.mark.parametrize("hops", [0, 3, 4, 29, 30, 31])
def test_rows_either_side_of_where_each_window_begins(hops):
    x = noise(hops * H + 9, 20 + hops)
    rng = np.random.default_rng(950 + hops)
    _, _, _, last = check_against_one_shot(x, random_split(len(x), rng, most=3 * H), RATE, COEF)
    assert (last[0] > 0) == (hops >= 4) and (last[1] > 0) == (hops >= 4) and (last[2] > 0) == (hops >= 30) and last[4] == hops


def test_the_headers_own_example_of_a_peak_that_needs_the_finish():
    x = np.zeros(40, np.float32)
    x[-1] = 1.0
    calls, _, tail, last = check_against_one_shot(x, [40], RATE, COEF)
    assert calls[0][1] == 239 / 8192 and tail == 7964 / 8192 == last[3]
    calls, _, tail, _ = check_against_one_shot(x, [39, 1], RATE, COEF)
    assert calls[0][1] == 0 and calls[1][1] == 239 / 8192 and tail == 7964 / 8192


def test_refusals_of_the_model():
    m = RowModel(RATE, COEF, max_hops=2)
    assert m.next(noise(2 * H + 5, 30)) is not None
    before = m.read()
    assert m.next(noise(H - 5, 31)) is None and same_read(m.read(), before) and m.N == 2 * H + 5
    assert m.next(noise(H - 6, 31)) is not None
    m.finish()
    before = m.read()
    assert m.next(noise(1, 32)) is None and m.finish() == 0.0
    idle = m.next(noise(0, 32))
    assert len(idle[0]) == 0 and bits(idle[1]) == bits(0.0) and idle[2] == 0 and same_read(m.read(), before)


# ---- grail_meter_stream_hops ----------------------------------------------------------------------------------------------------
def test_meter_stream_hops_against_integer_arithmetic(built):
    rng = np.random.default_rng(960)
    lib = G.load()
    for rate in (2560, 2569, 8000, 44100, 48000, 1048576):
        h = rate // 10
        for fed in (0, 1, h - 1, h, h + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - h, 2 ** 63, 2 ** 64 - 1 - 5 * h):
            for n in (0, 1, h - 1, h, 5 * h, int(rng.integers(0, 2 ** 32))):
                if fed + n < 2 ** 64:
                    assert G.meter_stream_hops(fed, n, rate) == hops_of_call(fed, n, h), (rate, fed, n)
    out = C.c_uint64(77)
    for args in ((0, 1, 2559), (0, 1, 1048577), (0, 1, 0), (2 ** 64 - 1, 1, 48000), (1, 2 ** 64 - 1, 48000)):
        assert lib.grail_meter_stream_hops(*args, C.addressof(out)) == G.ERR_INVALID_ARG and out.value == 77, args
    assert lib.grail_meter_stream_hops(0, 1, 48000, None) == G.ERR_INVALID_ARG
    assert G.meter_stream_hops(2 ** 64 - 2, 1, 48000) == hops_of_call(2 ** 64 - 2, 1, 4800)


# ---- every host refusal, with no device needed ------------------------------------------------------------------------------------
def answer(name, *args):
    lib = G.load()
    status = getattr(lib, name)(None, *args)
    message = lib.grail_last_error().decode()
    if status == G.ERR_NO_DEVICE or (status == G.ERR_INVALID_ARG and message == name + ": ctx is NULL"):
        return PAST
    assert status == G.ERR_INVALID_ARG, (name, args, status, message)
    assert message.startswith(name + ": "), message
    return message[len(name) + 2:]


def test_open_says_what_is_wrong_with_its_numbers_first(built):
    name, out = "grail_meter_stream_open", C.c_void_p(0x77)
    at = C.addressof(out)
    rate_words = "sample_rate is outside GRAIL_LOUDNESS_RATE_MIN .. GRAIL_LOUDNESS_RATE_MAX"
    assert answer(name, 1, 2559, None, 10, at) == rate_words and answer(name, 1, 1048577, None, 10, at) == rate_words
    assert answer(name, 0, 48000, None, 10, at) == "n_rows is 0"
    assert answer(name, 1, 48000, None, 0, at) == "max_hops is 0"
    too_many = "n_rows x max_hops x 8 bytes of ledger do not fit size_t"
    assert answer(name, 2, 48000, None, 2 ** 60, at) == too_many and answer(name, 1, 48000, None, 2 ** 61, at) == too_many
    assert answer(name, 2 ** 32 - 1, 48000, None, 2 ** 29 + 1, at) == too_many
    # numbers that are fine: without a context there is nothing to open
    assert answer(name, 2, 48000, None, 2 ** 60 - 1, at) == "NULL argument" and answer(name, 4, 2560, None, 1, None) == "NULL argument"
    assert out.value == 0x77


def test_next_refusals_in_their_order(built):
    name = "grail_meter_stream_next_async"
    nothing = (None, None, None)
    assert answer(name, None, IN, 64, LEN, None, 0, *nothing) == "the stream is NULL"
    # (without a context: the checks of one row at the smallest hop, 256)
    assert answer(name, HANDLE, IN, 64, None, None, 0, *nothing) == "NULL buffer"
    assert answer(name, HANDLE, None, 64, LEN, None, 0, *nothing) == "NULL buffer"
    assert answer(name, HANDLE, None, 0, None, None, 0, *nothing) == "NULL buffer"
    assert answer(name, HANDLE, None, 0, LEN, None, 0, *nothing) == PAST            # rows of no samples: only in_len is needed
    assert answer(name, HANDLE, IN, 2 ** 60 + 1, LEN, None, 0, *nothing) == "the rows span more than 2^60 samples"
    stride_words = "hops_stride < (in_stride + H - 1) / H, the most hops a call can complete"
    assert answer(name, HANDLE, IN, 256, LEN, OUT, 0, *nothing) == stride_words
    assert answer(name, HANDLE, IN, 257, LEN, OUT, 1, *nothing) == stride_words
    assert answer(name, HANDLE, IN, 1, LEN, OUT, 0, *nothing) == stride_words
    assert answer(name, HANDLE, IN, 64, LEN, OUT, 2 ** 60 + 1, *nothing) == "the rows span more than 2^60 samples"
    for args in ((IN, 256, LEN, OUT, 1), (IN, 257, LEN, OUT, 2), (IN, 1, LEN, OUT, 1), (IN, 257, LEN, None, 0), (IN, 2 ** 60, LEN, None, 0),
                 (IN, 2 ** 32 + 5, LEN, OUT, 2 ** 24 + 1)):
        assert answer(name, HANDLE, *args, *nothing) == PAST, args


def test_read_ledger_finish_and_close_refusals(built):
    five = (None,) * 5
    assert answer("grail_meter_stream_read_async", None, *five) == "the stream is NULL"
    assert answer("grail_meter_stream_read_async", HANDLE, *five) == PAST
    assert answer("grail_meter_stream_finish_async", None, None, None) == "the stream is NULL"
    assert answer("grail_meter_stream_finish_async", HANDLE, None, None) == PAST
    assert answer("grail_meter_stream_finish_async", HANDLE, LEN, OUT) == PAST
    base, stride = C.c_void_p(0x77), C.c_uint64(0x77)
    assert answer("grail_meter_stream_ledger", None, C.addressof(base), C.addressof(stride)) == "the stream is NULL"
    assert answer("grail_meter_stream_ledger", HANDLE, None, C.addressof(stride)) == "NULL argument"
    assert answer("grail_meter_stream_ledger", HANDLE, C.addressof(base), None) == "NULL argument"
    assert answer("grail_meter_stream_ledger", HANDLE, C.addressof(base), C.addressof(stride)) == PAST
    assert base.value == 0x77 and stride.value == 0x77
    lib = G.load()
    assert lib.grail_meter_stream_close(None, None) == G.OK                      # no stream: a no-op, as the other kinds'
    assert answer("grail_meter_stream_close", HANDLE) == PAST


def test_the_headers_new_functions_are_exported(built):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "grail_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(grail_meter_stream_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(["grail_meter_stream_hops", "grail_meter_stream_open", "grail_meter_stream_next_async",
                               "grail_meter_stream_read_async", "grail_meter_stream_ledger", "grail_meter_stream_finish_async",
                               "grail_meter_stream_close"])
    lib = G.load()
    for name in declared:
        assert hasattr(lib, name) and name in G.EXPORTS, name
    assert G.LIMIT_REFUSED == REFUSED and re.search(r"#define GRAIL_ABI_VERSION 4\b", open(os.path.join(root, "include", "grail_hip.h")).read())


def test_every_line_of_the_census_names_a_test_that_exists():
    """tests/KERNEL_PATHS_METER_STREAM.md: every row names, in its last column, test ids `file.py::name` that exist, and every
    kernel of the file has a row"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "KERNEL_PATHS_METER_STREAM.md")) as f:
        rows = [line for line in f if line.startswith("|") and not re.match(r"\|\s*(-+|kernel)\s*\|", line)]
    assert len(rows) >= 12
    for line in rows:
        ids = re.findall(r"`(test_\w+\.py)::(test_\w+)", line.rstrip().rstrip("|").split("|")[-1])
        assert ids, "a line without a test id: " + line
        for name, test in ids:
            with open(os.path.join(root, "tests", name)) as src:
                assert re.search(r"^def " + test + r"\(", src.read(), flags=re.M), (name, test)
    named = " ".join(line.split("|")[1] for line in rows)
    for kernel in ("meter_stream_hops_kernel<true>", "meter_stream_hops_kernel<false>", "meter_stream_peak_kernel<true>",
                   "meter_stream_peak_kernel<false>", "meter_stream_advance_kernel", "meter_stream_read_kernel"):
        assert kernel in named, kernel


def test_stream_model_and_row_model_agree():
    x = noise(3 * H + 1, 40)
    calls, reads, tail, last = stream_model(x, [H + 1, 0, 2 * H], RATE, COEF)
    m = RowModel(RATE, COEF)
    for n, at, c, r in zip([H + 1, 0, 2 * H], [0, H + 1, H + 1], calls, reads):
        got = m.next(x[at:at + n])
        assert np.array_equal(bits(got[0]), bits(c[0])) and bits(got[1]) == bits(c[1]) and got[2] == c[2] and same_read(m.read(), r)
    assert bits(m.finish()) == bits(tail) and same_read(m.read(), last)
