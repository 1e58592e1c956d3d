"""The C++ facade (include/grail.hpp) on the device, method by method: tests/facade_driver.cpp runs one group of facade calls
per child process over inputs written here, and everything it returns is compared here with the models the GPU tests of the
C ABI use — bit for bit unless a test says otherwise.  A wrong stride, a group index or a length cut in the header's host code
returns another row's samples; the rows of every call differ, so that shows.

Each group is one run of the driver (a module-scoped fixture); the tests compare parts of that run.  If a run ends by a signal,
by status 134 or 139 or at its time limit, every later fixture of this file skips: nothing more is started on the device."""
import struct
import time

import numpy as np
import pytest

import grail_hip as G
import oracle_lib as O
from fir_model import fir_model
from fir_stream_model import stream_len as fir_stream_len
from grail_hip import workload as W
from limit_stream_model import delay as limit_delay, stream_len as limit_stream_len
from resample_model import resample_model
from resample_stream_model import stream_len as resample_stream_len
from test_facade_host import (FAULT_STATUSES, build_driver, get, get_rows, put, put_manifest, put_rows, run_driver, same)
from test_levels_host import row_model
from test_limiter_host import REFUSED, limiter_model
from test_loudness_host import gate_model, kweight_hops_model
from test_loudness_segmented_host import segmented_hops_model
from test_mix_gpu import fold, same_bits
from test_true_peak_host import true_peak_model

pytestmark = pytest.mark.gpu
CEILING, ELL = np.float32(0.5), 3
_faulted = []


def noise(rng, n, bad=()):
    """uniform noise with a -0.0 in it; bad: (index, value) pairs of non-finite samples to plant"""
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    if n > 2:
        x[n // 3] = np.float32(-0.0)
    for i, v in bad:
        x[i] = np.float32(v)
    return x


@pytest.fixture(scope="module")
def driver(built, tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("facade_driver"))


def run_group(driver, group, folder):
    """one run of the driver as a fresh child -> the folder of its outputs"""
    if _faulted:
        pytest.skip(f"the driver's run of group {_faulted[0]} faulted: nothing more is started on the device")
    out = folder / "out"
    out.mkdir()
    t0 = time.perf_counter()
    r = run_driver(driver, group, folder, out)
    wall = time.perf_counter() - t0
    if r.returncode is None or r.returncode < 0 or r.returncode in FAULT_STATUSES:
        _faulted.append(group)
    assert r.returncode == 0, (group, r.returncode, r.stderr)
    print(f"facade_driver {group}: {wall:.2f} s wall")
    return out


# ---- group rows ------------------------------------------------------------------------------------------------------------
ROW_LENS = [0, 1, 64, 65, 1000]
LD_RATE, TL_RATES = 8000, {"tl": 2560, "tl2": 5120}
PAIRS = [(48000, 16000), (44100, 48000)]
FILTERS = [(1, 0), (9, 4), (40, 39)]             # (K, origin)
WHICH = [0, 2, 1, 7, 0]


@pytest.fixture(scope="module")
def rows_in():
    rng = np.random.default_rng(7001)
    d = dict(
        lv=[noise(rng, n) for n in ROW_LENS[:4]] + [noise(rng, 1000, [(10, np.nan), (500, np.inf), (999, -np.inf)])],
        tp=[noise(rng, n) for n in ROW_LENS] + [noise(rng, 4097, [(4096, np.nan), (7, np.inf)])],
        ld=[noise(rng, 0), noise(rng, 799), noise(rng, 3200, [(5, np.nan)]), noise(rng, 5000, [(4000, np.inf)])],
        tl=[noise(rng, 0), noise(rng, 255), noise(rng, 4 * 256 + 3, [(1000, np.nan)]), noise(rng, 33 * 256 + 100, [(0, np.inf)])],
        tl2=[noise(rng, 0), noise(rng, 511), noise(rng, 4 * 512 + 3, [(2000, np.nan)]), noise(rng, 33 * 512 + 100, [(0, np.inf)])],
        lim1=[noise(rng, 300), noise(rng, 1000, [(17, np.nan)]), noise(rng, 65)],
        lim2=[noise(rng, 700), noise(rng, 700, [(699, np.inf)]), noise(rng, 900), noise(rng, 899)],
        rs=[noise(rng, 0), noise(rng, 1), noise(rng, 65), noise(rng, 1500)],
        fr=[noise(rng, 1000), noise(rng, 65), noise(rng, 0), noise(rng, 64), noise(rng, 333)],
        taps=[rng.uniform(-1.0, 1.0, K).astype(np.float32) for K, _ in FILTERS])
    for v in d.values():
        for x in v:
            x.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def rows_out(driver, rows_in, tmp_path_factory):
    folder = tmp_path_factory.mktemp("facade_rows")
    for name in ("lv", "tp", "ld", "tl", "tl2", "lim1", "lim2", "rs", "fr"):
        put_rows(folder, name, rows_in[name])
    put_rows(folder, "firset", rows_in["taps"])
    put(folder, "firset.origin.u32", [o for _, o in FILTERS], "u4")
    put_manifest(folder, **{"ld.rate": LD_RATE, "tl.rate": TL_RATES["tl"], "tl2.rate": TL_RATES["tl2"], "ceiling": float(CEILING),
                            "lookahead_log2": ELL, "rs.pairs": [r for p in PAIRS for r in p], "fr.which": WHICH})
    return run_group(driver, "rows", folder)


def test_levels_of_five_rows_in_one_call(rows_in, rows_out):
    want = [row_model(x) for x in rows_in["lv"]]
    assert same(get(rows_out, "lv.sumsq.f64", "f8"), [w[0] for w in want], np.float64)
    assert same(get(rows_out, "lv.peak.f32", "f4"), [w[1] for w in want])
    assert list(get(rows_out, "lv.bad.u32", "u4")) == [w[2] for w in want] == [0, 0, 0, 0, 3]
    assert list(get(rows_out, "lv.none.u32", "u4")) == [0, 0, 0]


@pytest.mark.parametrize("name", ["lv", "tp"])
def test_true_peak(rows_in, rows_out, name):
    want = [true_peak_model(x) for x in rows_in[name]]
    got = get(rows_out, name + ".tp.f64", "f8")
    assert same(got, [w[0] for w in want], np.float64)
    assert list(get(rows_out, name + ".tpbad.u32", "u4")) == [w[1] for w in want]
    assert same(get(rows_out, name + ".tpdb.f64", "f8"), [G.true_peak_db(t) for t in got], np.float64)
    assert got[0] == 0 and got[-1] > 0 and want[-1][1] >= 2


def test_loudness_the_serial_form(rows_in, rows_out):
    H = LD_RATE // 10
    want = [(gate_model(h, H), b) for h, b in kweight_hops_model(rows_in["ld"], LD_RATE, G.kweighting(LD_RATE))]
    got = get(rows_out, "ld.ms.f64", "f8")
    assert same(got, [w[0] for w in want], np.float64)
    assert list(get(rows_out, "ld.bad.u32", "u4")) == [w[1] for w in want] == [0, 0, 1, 1]
    assert same(get(rows_out, "ld.lufs.f64", "f8"), [G.loudness_lufs(g) for g in got], np.float64)
    assert got[0] == 0 and got[1] == 0 and got[2] > 0 and got[3] > 0        # 799 samples: under 400 ms


def nan_or_same(a, b):
    """bit for bit, but any NaN equals any NaN (its sign and payload are the arithmetic unit's own)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


@pytest.mark.parametrize("name", ["tl", "tl2"])
def test_track_loudness_and_what_a_meter_reads_from_its_hops(rows_in, rows_out, name):
    """At 2 560 Hz the rate's own shelf lies above half the rate: its filter grows without bound, the hop sums run to Inf (and
    the gate to NaN) in the model and on the device alike; the row cuts and the hop count are what that case holds.  At
    5 120 Hz every number is finite and the meter's readings mean something."""
    rate = TL_RATES[name]
    H = rate // 10
    with np.errstate(all="ignore"):
        want = segmented_hops_model(rows_in[name], rate, G.kweighting(rate))
        gated = [gate_model(wh, H) for wh, _ in want]
    hops = get_rows(rows_out, name + ".hops", "f8", ".f64")
    assert list(get(rows_out, name + ".hop.u32", "u4")) == [H]
    assert [len(h) for h in hops] == [len(x) // H for x in rows_in[name]] == [0, 0, 4, 33]
    for i, (wh, wb) in enumerate(want):
        assert nan_or_same(hops[i], wh), i
    assert nan_or_same(get(rows_out, name + ".ms.f64", "f8"), gated)
    assert list(get(rows_out, name + ".bad.u32", "u4")) == [wb for _, wb in want] == [0, 0, 1, 1]
    assert nan_or_same(get(rows_out, name + ".range.f64", "f8"), [G.loudness_range(h, H) for h in hops])
    assert nan_or_same(get(rows_out, name + ".momentary.f64", "f8"), [G.loudness_lufs(G.loudness_window_max(h, H, 4)) for h in hops])
    short_term = get(rows_out, name + ".short_term.f64", "f8")
    assert nan_or_same(short_term, [G.loudness_lufs(G.loudness_window_max(h, H, 30)) for h in hops])
    assert short_term[2] == -np.inf
    if name == "tl2":
        assert all(np.isfinite(h).all() for h in hops) and np.isfinite(short_term[3]) and get(rows_out, name + ".range.f64", "f8")[3] > 0


def check_limited(folder, name, rows, group):
    out, gain, nlim, bad = limiter_model(rows, CEILING, ELL, group=group)
    got = get_rows(folder, name + ".out")
    assert len(got) == len(rows)
    for i, z in enumerate(got):
        if out[i] is None:
            assert len(z) == 0, (name, i)
        else:
            assert same(z, out[i]), (name, i)
    refused = nlim == REFUSED
    got_gain = get(folder, name + ".gain.f32", "f4")
    assert same(got_gain[~refused], gain[~refused]) and np.isnan(got_gain[refused]).all()
    assert np.array_equal(get(folder, name + ".nlim.u32", "u4"), nlim)
    assert np.array_equal(get(folder, name + ".bad.u32", "u4"), bad)
    assert np.array_equal(get(folder, name + ".refused.u32", "u4"), refused.astype(np.uint32))
    return nlim, bad


def test_limit_three_rows_each_its_own_group(rows_in, rows_out):
    nlim, bad = check_limited(rows_out, "lim1", rows_in["lim1"], 1)
    assert (nlim > 0).all() and list(bad) == [0, 1, 0]


def test_limit_a_served_pair_and_a_refused_pair(rows_in, rows_out):
    nlim, bad = check_limited(rows_out, "lim2", rows_in["lim2"], 2)
    assert 0 < nlim[0] < REFUSED and nlim[1] == REFUSED and bad[0] == 1
    assert [len(z) for z in get_rows(rows_out, "lim2.out")] == [700, 700, 0, 0]


@pytest.mark.parametrize("k", range(len(PAIRS)))
def test_resample(rows_in, rows_out, k):
    rate_in, rate_out = PAIRS[k]
    num, (_, down, _) = G.resample_coefficients(rate_in, rate_out), G.resample_ratio(rate_in, rate_out)
    got = get_rows(rows_out, f"rs{k}.out")
    assert [len(y) for y in got] == [G.resample_len(len(x), rate_in, rate_out) for x in rows_in["rs"]]
    for i, x in enumerate(rows_in["rs"]):
        assert same(got[i], resample_model(x, num, down)[0]), (PAIRS[k], i)


@pytest.mark.parametrize("name,which,ring", [("ring", WHICH, True), ("plain", WHICH, False), ("first_ring", None, True),
                                             ("first_plain", None, False)])
def test_fir_with_a_which_vector_and_without_ringing_out_or_not(rows_in, rows_out, name, which, ring):
    got = get_rows(rows_out, f"fr.{name}.out")
    assert list(get(rows_out, "firset.facts.u32", "u4")) == [4, 40]           # the longest K - 1 - origin, the most taps
    for i, x in enumerate(rows_in["fr"]):
        f = which[i] if which else 0
        if f >= len(FILTERS):
            assert len(got[i]) == 0, i                                    # an index outside the set
            continue
        K, origin = FILTERS[f]
        want = fir_model(x, rows_in["taps"][f], origin)[0]
        assert len(want) == (len(x) + K - 1 - origin if len(x) else 0)
        assert same(got[i], want if ring else want[:len(x)]), (name, i)


def test_size_checks_throw_before_anything_is_queued(rows_out):
    """a `which` of another size than the rows, limit with n % group != 0, mix_leveled with one level too few,
    LimitStream::finish with one mark per row; and the two neighbours: group = 0, fir_stream with a short `which`"""
    assert list(get(rows_out, "throws.i32", "i4")) == [G.ERR_INVALID_ARG] * 6


# ---- group streams -------------------------------------------------------------------------------------------------------------
# how many samples each row is fed per call: a paused row beside fed ones, a call of 1 sample, a call longer than 64 (a stride
# of 128 while other rows hold less), a call in which every chunk is empty; after call 5 the marked units end, call 6 feeds them
# again (from their rows' start) beside their neighbours' last samples
SPLIT4 = np.array([[10, 0, 1, 70], [1, 1, 1, 1], [0, 0, 0, 0], [100, 30, 0, 5], [0, 64, 65, 0], [33, 7, 20, 64], [5, 40, 5, 13]])
SPLIT_PAIRS = np.array([[10, 10, 70, 70], [1, 1, 1, 1], [0, 0, 0, 0], [100, 100, 5, 5], [0, 0, 65, 65], [33, 33, 64, 64], [5, 5, 13, 13]])
FINISH_AFTER = 5
STREAM_FILTERS = [(9, 4), (40, 0)]
STREAM_WHICH = [0, 1, 1, 0]
STREAM_PAIRS = {"ra": (3, 2), "rb": (48000, 16000)}


def fed_lengths(split, marks, group=1):
    """the samples a row is fed while its unit is open"""
    ended = np.repeat(np.asarray(marks, bool), group)
    return [int(split[:FINISH_AFTER + 1, i].sum() + (0 if ended[i] else split[FINISH_AFTER + 1:, i].sum())) for i in range(split.shape[1])]


@pytest.fixture(scope="module")
def streams_in():
    rng = np.random.default_rng(7002)
    d = dict(fs=dict(split=SPLIT4, marks=[1, 0, 1, 0], group=1), ra=dict(split=SPLIT4[:, :3], marks=[1, 0, 1], group=1),
             rb=dict(split=SPLIT4[:, :3], marks=[1, 0, 1], group=1), ls=dict(split=SPLIT_PAIRS, marks=[1, 0], group=2))
    for s in d.values():
        s["rows"] = [noise(rng, n) for n in fed_lengths(s["split"], s["marks"], s["group"])]
        for x in s["rows"]:
            x.setflags(write=False)
    d["taps"] = [rng.uniform(-1.0, 1.0, K).astype(np.float32) for K, _ in STREAM_FILTERS]
    return d


@pytest.fixture(scope="module")
def streams_out(driver, streams_in, tmp_path_factory):
    folder = tmp_path_factory.mktemp("facade_streams")
    manifest = {"fs.which": STREAM_WHICH, "ceiling": float(CEILING), "lookahead_log2": ELL, "ls.group": 2, "ls.unequal_before": 3}
    for name in ("fs", "ra", "rb", "ls"):
        s = streams_in[name]
        put_rows(folder, name, s["rows"])
        put(folder, name + ".split.u32", s["split"], "u4")
        put(folder, name + ".marks.u32", s["marks"], "u4")
        manifest[name + ".finish_after"] = FINISH_AFTER
    for name, pair in STREAM_PAIRS.items():
        manifest[name + ".rates"] = list(pair)
    put_rows(folder, "fsset", streams_in["taps"])
    put(folder, "fsset.origin.u32", [o for _, o in STREAM_FILTERS], "u4")
    put_manifest(folder, **manifest)
    return run_group(driver, "streams", folder)


def check_stream(folder, name, s, whole, len_of):
    """The calls of one stream against whole[i], the model of row i in one piece, and len_of(i, fed_before, n, finishing),
    the count a call writes; -> the rows put together"""
    split, group = s["split"], s["group"]
    n, ended = split.shape[1], np.repeat(np.asarray(s["marks"], bool), group)
    fed, parts = [0] * n, [[] for _ in range(n)]
    for c in range(len(split)):
        got = get_rows(folder, f"{name}.call{c}")
        assert len(got) == n
        for i in range(n):
            if c > FINISH_AFTER and ended[i]:
                assert len(got[i]) == 0, (name, c, i, "an ended unit that is fed comes back empty")
                continue
            assert len(got[i]) == len_of(i, fed[i], int(split[c, i]), False), (name, c, i)
            parts[i].append(got[i])
            fed[i] += int(split[c, i])
    assert any(len(g) for g in get_rows(folder, f"{name}.call{len(split) - 1}"))      # ... and its neighbours are served
    some, rest, again = (get_rows(folder, f"{name}.finish_{k}") for k in ("some", "rest", "again"))
    for i in range(n):
        tail, other = (some, rest) if ended[i] else (rest, some)
        assert len(other[i]) == 0 and len(again[i]) == 0, (name, i)
        assert len(tail[i]) == len_of(i, fed[i], 0, True), (name, i)
        assert fed[i] == len(s["rows"][i])
        joined = np.concatenate(parts[i] + [tail[i]])
        assert same(joined, whole[i]), (name, i, "the calls end to end and the tail are not the row in one piece")
        # a fresh stream move-assigned onto the used one: the whole row in one call, then its tail
        moved = np.concatenate([get_rows(folder, f"{name}.moved.call")[i], get_rows(folder, f"{name}.moved.finish")[i]])
        assert same(moved, whole[i]), (name, i, "moved")
    return [np.concatenate(parts[i]) for i in range(n)]


def test_fir_stream_four_rows_on_two_filters(streams_in, streams_out):
    s = streams_in["fs"]
    filt = [STREAM_FILTERS[f] for f in STREAM_WHICH]
    whole = [fir_model(x, streams_in["taps"][f], STREAM_FILTERS[f][1])[0] for x, f in zip(s["rows"], STREAM_WHICH)]
    check_stream(streams_out, "fs", s, whole, lambda i, before, n, fin: fir_stream_len(before, n, filt[i][0], filt[i][1], fin))
    one_shot = get_rows(streams_out, "fs.oneshot")
    assert all(same(a, b) for a, b in zip(one_shot, whole)) and len(one_shot) == 4
    assert list(get(streams_out, "fs.rows.u32", "u4")) == [4, 39]


@pytest.mark.parametrize("name", ["ra", "rb"])
def test_resample_stream_three_rows(streams_in, streams_out, name):
    s, (rate_in, rate_out) = streams_in[name], STREAM_PAIRS[name]
    num, (up, down, taps) = G.resample_coefficients(rate_in, rate_out), G.resample_ratio(rate_in, rate_out)
    whole = [resample_model(x, num, down)[0] for x in s["rows"]]
    check_stream(streams_out, name, s, whole, lambda i, before, n, fin: resample_stream_len(before, n, up, down, taps, fin))
    one_shot = get_rows(streams_out, name + ".oneshot")
    assert all(same(a, b) for a, b in zip(one_shot, whole)) and len(one_shot) == 3
    assert list(get(streams_out, name + ".rows.u32", "u4")) == [3, -(-(taps // 2) * up // down)]


def test_limit_stream_two_linked_pairs(streams_in, streams_out):
    s = streams_in["ls"]
    whole = limiter_model(s["rows"], CEILING, ELL, group=2)[0]
    check_stream(streams_out, "ls", s, whole, lambda i, before, n, fin: limit_stream_len(before, n, ELL, fin))
    # the call that fed the members of group 0 three and two samples: both come back empty, nothing of the group moved
    # (what followed continued to the one-shot bits, above), and the other group was not fed
    assert [len(z) for z in get_rows(streams_out, "ls.unequal")] == [0, 0, 0, 0]
    one_shot = get_rows(streams_out, "ls.oneshot.out")
    assert all(same(a, b) for a, b in zip(one_shot, whole)) and len(one_shot) == 4
    assert list(get(streams_out, "ls.facts.u32", "u4")) == [4, 2, limit_delay(ELL)] and limit_delay(ELL) == G.limit_stream_delay(ELL)
    assert list(get(streams_out, "ls.rows.u32", "u4")) == [4, limit_delay(ELL)]
    assert (limiter_model(s["rows"], CEILING, ELL, group=2)[2] > 0).all()          # the curves are at work


def test_limit_stream_finish_async_writes_the_tail_where_the_caller_says(streams_in, streams_out):
    row = streams_in["ls"]["rows"][0]
    head, tail = get_rows(streams_out, "ls.async")
    assert len(tail) == limit_delay(ELL) and len(head) == len(row) - limit_delay(ELL)
    assert same(np.concatenate([head, tail]), limiter_model([row], CEILING, ELL)[0][0])


# ---- group chain -------------------------------------------------------------------------------------------------------------
CHUNK, N_TRACKS, TRACK_LEN, WAV_RATE, LIVE_CHUNK = 100, 2, 5003, 22050, 300


def utterances(rng, counts, vids, seeds):
    """utterances of counts[u] short segments (0.01 - 0.02 s) -> (segs, offs, vids, seeds)"""
    per = []
    for u, k in enumerate(counts):
        ph = rng.choice([G.PH_A, G.PH_E, G.PH_SILENCE, G.PH_STOP], size=k, p=[0.45, 0.4, 0.1, 0.05])
        hz = rng.uniform(90.0, 220.0, size=k) / 44100.0
        per.append(G.segments([(int(ph[i]), float(rng.uniform(0.01, 0.02)), 0.0078125, float(hz[i])) for i in range(k)]))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return np.concatenate(per), offs, np.asarray(vids, np.uint32), np.asarray(seeds, np.uint32)


def put_utterances(folder, name, batch):
    segs, offs, vids, seeds = batch
    put(folder, name + ".segs.bin", np.frombuffer(segs.tobytes(), np.uint8))
    put(folder, name + ".offs.u32", offs, "u4")
    put(folder, name + ".vids.u32", vids, "u4")
    put(folder, name + ".seeds.u32", seeds, "u4")


def oracle_rows(voices, batch):
    ov = [O.Voice.from_buffer_copy(bytes(v)) for v in voices]
    counts = O.count_batch(ov, *batch)
    stride = (int(np.max(counts, initial=1)) + 63) // 64 * 64
    out, lens = O.synthesize_batch(ov, *batch, stride)
    return [out[u, :lens[u]].copy() for u in range(len(lens))]


def as_matrix(rows):
    m = np.zeros((len(rows), max(max(len(r) for r in rows), 1)), np.float32)
    for i, r in enumerate(rows):
        m[i, :len(r)] = r
    return m, np.array([len(r) for r in rows], np.uint32)


@pytest.fixture(scope="module")
def chain_in(built):
    rng = np.random.default_rng(7003)
    voices = W.preset_voices(2)
    d = dict(voices=voices,
             syn=utterances(rng, [3, 1, 0, 5, 2], [0, 1, 0, 1, 1], [0, 7, 8, 0xFFFFFFFF, 12345]),
             mix=utterances(rng, [4, 2, 5], [1, 0, 1], [3, 4, 5]),
             lev=utterances(rng, [3, 0, 5, 2], [0, 1, 1, 0], [6, 7, 8, 9]),
             live=utterances(rng, [3, 2, 4], [1, 1, 1], [9, 9, 9]),
             mix_place=np.array([[0, 0, 0], [1, 0, 100], [2, 1, 50], [0, 1, 300]], np.uint32),
             mix_gain=np.array([1.0, 0.5, -0.75, 0.25], np.float32),
             lev_place=np.array([[0, 0, 0], [1, 0, 10], [2, 1, 64], [3, 0, 700], [0, 1, 1000], [2, 0, 2000]], np.uint32),
             level_db=np.array([-20.0, -20.0, -23.0, -18.0, -26.0, -12.0], np.float32))
    d["wav"] = [noise(rng, 1000, [(3, np.nan)]) * np.float32(1.5), noise(rng, 777), noise(rng, 777) * np.float32(2.0), noise(rng, 776)]
    # the ceiling at the median of what the leveled placements would reach, from the oracle's rows: some are cut back, some not
    rows = oracle_rows(voices, d["lev"])
    measured = [row_model(r) for r in rows]
    leveled, _ = G.level_gains(G.LEVEL_RMS, d["lev_place"][:, 0], d["level_db"], sumsq=[m[0] for m in measured],
                               nonfinite=[m[2] for m in measured], row_len=[len(r) for r in rows])
    reach = leveled.astype(np.float64) * np.array([true_peak_model(r)[0] for r in rows])[d["lev_place"][:, 0]]
    d["ceiling_db"] = float(np.float32(20.0 * np.log10(np.median(reach[reach > 0]))))
    return d


@pytest.fixture(scope="module")
def chain_out(driver, chain_in, tmp_path_factory):
    folder = tmp_path_factory.mktemp("facade_chain")
    put(folder, "voices.bin", np.frombuffer(b"".join(bytes(v) for v in chain_in["voices"]), np.uint8))
    for name in ("syn", "mix", "lev", "live"):
        put_utterances(folder, name, chain_in[name])
    for name, place, gain in (("mix", chain_in["mix_place"], chain_in["mix_gain"]),
                              ("lev", chain_in["lev_place"], np.ones(len(chain_in["lev_place"]), np.float32))):
        put(folder, name + ".place.u32", place, "u4")
        put(folder, name + ".gain.f32", gain, "f4")
    put(folder, "lev.level_db.f32", chain_in["level_db"], "f4")
    put_rows(folder, "wav", chain_in["wav"])
    put_manifest(folder, **{"chunk": CHUNK, "n_tracks": N_TRACKS, "track_len": TRACK_LEN, "ceiling_db": chain_in["ceiling_db"],
                            "wav.rate": WAV_RATE, "live.chunk": LIVE_CHUNK})
    return run_group(driver, "chain", folder)


def test_synthesize_five_utterances_over_two_voices(chain_in, chain_out):
    want = oracle_rows(chain_in["voices"], chain_in["syn"])
    got = get_rows(chain_out, "syn.out")
    assert [len(r) for r in got] == [len(r) for r in want] and len(want[2]) == 0 and len(set(len(r) for r in want)) == 5
    assert all(same(a, b) for a, b in zip(got, want))
    assert list(get(chain_out, "syn.lengths.u32", "u4")) == [len(r) for r in want]
    assert list(get(chain_out, "voices.count.u32", "u4")) == [2]


def test_stream_in_chunks_of_100_is_synthesize(chain_out):
    whole, joined = get_rows(chain_out, "syn.out"), get_rows(chain_out, "stream.out")
    assert len(joined) == len(whole) == 5 and all(same(a, b) for a, b in zip(joined, whole))
    pulls, longest, of_nothing, n_chunks = get(chain_out, "stream.facts.u32", "u4")
    assert pulls == -(-max(len(r) for r in whole) // CHUNK) and longest == CHUNK
    assert of_nothing == 0 and n_chunks == 0                                 # a Stream of no utterances: false at once


def test_fast_arithmetic_and_back(gpu_ctx, chain_in, chain_out):
    want = oracle_rows(chain_in["voices"], chain_in["syn"])
    fast, again = get_rows(chain_out, "fast.out"), get_rows(chain_out, "exact_again.out")
    assert [len(r) for r in fast] == [len(r) for r in want]
    worst = max(float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)), initial=0.0)) for a, b in zip(fast, want))
    assert worst <= G.FAST_TOLERANCE
    assert all(same(a, b) for a, b in zip(again, want))
    gpu_ctx.set_voices(chain_in["voices"])
    try:
        served = gpu_ctx.get_option("fast_arithmetic_served")
    finally:
        gpu_ctx.set_voices(W.single_voice())
    assert list(get(chain_out, "fast.served.u32", "u4")) == [served, served]
    print(f"fast arithmetic through the facade: served = {served}, max |d| = {worst * 2.0 ** 23:.1f} * 2^-23")


def placed(place, gains, rows):
    m, lens = as_matrix(rows)
    return fold(m, lens, place[:, 0], place[:, 1], place[:, 2].astype(np.uint64), gains, N_TRACKS, TRACK_LEN)


def test_mix_overlapping_placements_on_two_tracks(chain_in, chain_out):
    rows = get_rows(chain_out, "mix.rows")
    assert all(same(a, b) for a, b in zip(rows, oracle_rows(chain_in["voices"], chain_in["mix"])))
    got = np.array(get_rows(chain_out, "mix.out"))
    assert got.shape == (N_TRACKS, TRACK_LEN)
    assert same_bits(got, placed(chain_in["mix_place"], chain_in["mix_gain"], rows))
    assert len(rows[0]) > 300 and len(rows[1]) > 0 and np.abs(got).max() > 0          # the placements overlap


def expected_gains(chain_in, rows, limited):
    measured = [row_model(r) for r in rows]
    place = chain_in["lev_place"]
    gains, unleveled = G.level_gains(G.LEVEL_RMS, place[:, 0], chain_in["level_db"], sumsq=[m[0] for m in measured],
                                     nonfinite=[m[2] for m in measured], row_len=[len(r) for r in rows])
    if not limited:
        return gains, unleveled, 0
    gains, cut = G.true_peak_limit_gains([true_peak_model(r)[0] for r in rows], place[:, 0], gains, chain_in["ceiling_db"])
    return gains, unleveled, cut


@pytest.mark.parametrize("name,limited", [("lev", False), ("levlim", True)])
def test_mix_leveled_gains_counts_and_tracks(chain_in, chain_out, name, limited):
    rows = get_rows(chain_out, "lev.rows")
    assert all(same(a, b) for a, b in zip(rows, oracle_rows(chain_in["voices"], chain_in["lev"]))) and len(rows[1]) == 0
    want, unleveled, cut = expected_gains(chain_in, rows, limited)
    gains = get(chain_out, name + ".gains.f32", "f4")
    assert same(gains, want), (gains, want)
    assert list(get(chain_out, name + ".counts.u32", "u4")) == ([unleveled, cut] if limited else [unleveled])
    assert unleveled == 1 and gains[1] == 0 and (0 < cut < len(gains) if limited else True)
    got = np.array(get_rows(chain_out, name + ".out"))
    assert got.shape == (N_TRACKS, TRACK_LEN) and same_bits(got, placed(chain_in["lev_place"], gains, rows))
    if not limited:
        assert same_bits(got, np.array(get_rows(chain_out, "lev.plain.out")))      # the same without the out-parameters


def wav_fields(raw):
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data"
    return struct.unpack("<I", raw[4:8]) + struct.unpack("<IHHIIHH", raw[16:36]) + struct.unpack("<I", raw[40:44])


def pcm16(x):
    L = O.lib()
    return np.array([L.orc_pcm16(float(v)) if not np.isnan(v) else 0 for v in x], dtype="<i2")


def test_save_wav_and_save_wav_frames(chain_in, chain_out):
    mono, left, right, _ = chain_in["wav"]
    raw = get(chain_out, "mono.wav", "u1").tobytes()
    assert wav_fields(raw) == (36 + 2 * len(mono), 16, 1, 1, WAV_RATE, 2 * WAV_RATE, 2, 16, 2 * len(mono))
    assert raw[44:] == pcm16(mono).tobytes() and np.nanmax(np.abs(mono)) > 1.0 and np.isnan(mono).any()
    raw = get(chain_out, "stereo.wav", "u1").tobytes()
    assert wav_fields(raw) == (36 + 4 * len(left), 16, 1, 2, WAV_RATE, 4 * WAV_RATE, 4, 16, 4 * len(left))
    assert raw[44:] == np.stack([pcm16(left), pcm16(right)], axis=1).tobytes()
    assert list(get(chain_out, "wav.throws.i32", "i4")) == [G.ERR_INVALID_ARG]      # tracks of different lengths


def test_live_stream_is_one_chain(chain_in, chain_out):
    segs, offs, vids, seeds = chain_in["live"]
    ov = O.Voice.from_buffer_copy(bytes(chain_in["voices"][int(vids[0])]))
    want, n = O.synthesize_phonemes(ov, segs, int(seeds[0]))
    got = get(chain_out, "live.out.f32", "f4")
    assert len(got) == n and same(got, want)
    pending, pulled = get(chain_out, "live.pending.u32", "u4"), get(chain_out, "live.pulled.u32", "u4")
    assert pending[0] == 0 and pending[1] == offs[1] and (pending <= len(segs)).all()
    assert pulled.max() == LIVE_CHUNK and pulled[-1] == 0 and int(pulled.sum()) == n
    assert list(get(chain_out, "live.chunk.u32", "u4")) == [LIVE_CHUNK]
