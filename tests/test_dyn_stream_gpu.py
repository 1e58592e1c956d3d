"""Dynamics streams on the device (grail_dyn_stream_*) against grail_dyn_async on the whole rows, bit for bit: 70 rows (a whole
wave and a partial one) on three curves, fed in calls of 1, 63, 64, 65, 0 and 300 samples with the rows advancing by different
amounts in one call (some paused, some ended early), self-keyed and keyed (two rows on one key among them).  The outputs of
the calls put end to end are the one-shot rows, the calls' non-finite counts add up to its count, the smallest of the calls'
min_gain among those that fed the row something is its min_gain, and a call that feeds a row nothing reads 1.0.  Both are held to the numpy model as well.  Then what
only a live stream can be asked: a set with an open stream refuses grail_dyn_free, close then free succeeds, and the calls a
keyed or self-keyed stream refuses."""
import ctypes as C

import numpy as np
import pytest

import dyn_model as M
import grail_hip as G
from test_dyn_gpu import audio, run, same, same_bits, three_curves
from test_levels_gpu import CANARY, Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
N_ROWS = 70
STEPS = (1, 63, 64, 65, 0, 300)


def corpus(keyed):
    rng = np.random.default_rng(21 + keyed)
    n = [int(v) for v in rng.integers(0, 494, N_ROWS)]
    n[0], n[1], n[2], n[69] = 493, 0, 64, 493                  # (1 + 63 + 64 + 65 + 0 + 300 = 493: the longest a row can be)
    rows = [audio(k, rng) for k in n]
    rows[0][[5, 200]] = (np.nan, np.inf)
    which = [int(v) for v in rng.integers(0, 3, N_ROWS)]
    if not keyed:
        return rows, which, None, None
    # 69 keys: rows 0 and 69, equally long and fed alike, listen to key 0 (the rows on one key advance together: a call's key
    # is read from where the rows it drives stand); every other row has a key of its own
    key_row = [0] + [int(v) for v in rng.permutation(np.arange(1, N_ROWS - 1))] + [0]
    keys = [audio(493, rng) for _ in range(N_ROWS - 1)]
    keys[0][7] = np.nan
    return rows, which, keys, key_row


@pytest.mark.parametrize("keyed", [False, True], ids=["self-keyed", "keyed"])
def test_any_chunking_gives_the_one_shot_rows(gpu_ctx, dev, keyed):
    rows, which, keys, key_row = corpus(keyed)
    n = [len(x) for x in rows]
    curves = three_curves()
    dyn_set = gpu_ctx.dyn_create(curves)
    # the one shot: on the device and in the model (a stream's key is as long as the row it drives)
    key_lens = None if not keyed else [n[key_row.index(k)] for k in range(N_ROWS - 1)]
    want = M.dyn_model(rows, curves, which, keys=keys, key_row=key_row, key_lens=key_lens)
    whole = run(gpu_ctx, dev, dyn_set, rows, which, keys=keys, key_row=key_row, key_lens=key_lens)
    same(want, whole, "one shot")
    st = gpu_ctx.dyn_stream_open(dyn_set, N_ROWS, which, N_ROWS - 1 if keyed else 0, key_row)
    with pytest.raises(G.GrailError):                           # the set has an open stream
        gpu_ctx.dyn_free(dyn_set)
    at = [0] * N_ROWS
    pieces = [[] for _ in range(N_ROWS)]
    bad = np.zeros(N_ROWS, np.int64)
    mg = np.full(N_ROWS, np.inf)
    for call, step in enumerate(STEPS):
        # rows advance by different amounts: every third row lags a call behind with half a step
        feed = [min(step if (r + call) % 3 else step // 2, n[r] - at[r]) for r in range(N_ROWS)]
        assert feed[69] == feed[0]                              # (the two rows on one key are fed alike)
        if call == len(STEPS) - 1:
            feed = [n[r] - at[r] for r in range(N_ROWS)]      # the rest (at most 300 + what lagging left)
        stride = max(max(feed), 1)
        stride += call                                          # (strides of every residue mod 4: both paths)
        host = np.full(N_ROWS * stride, np.nan, np.float32)
        for r in range(N_ROWS):
            host[r * stride:r * stride + feed[r]] = rows[r][at[r]:at[r] + feed[r]]
        d_in, d_len = dev.up(host), dev.up(np.array(feed, np.uint32))
        d_out = dev.up(np.full(N_ROWS * stride, CANARY, np.float32))
        kw = {}
        if keyed:
            khost = np.full((N_ROWS - 1) * stride, np.nan, np.float32)
            for r in range(N_ROWS):
                khost[key_row[r] * stride:key_row[r] * stride + feed[r]] = keys[key_row[r]][at[r]:at[r] + feed[r]]
            kw = dict(key_dev=dev.up(khost), key_stride=stride)
        out_len, nonfinite, gain = gpu_ctx.dyn_stream_next(st, N_ROWS, d_in, stride, d_len, d_out, stride, **kw)
        out = dev.down(d_out, (N_ROWS, stride), np.float32)
        for r in range(N_ROWS):
            assert out_len[r] == feed[r], (call, r)
            assert np.all(out[r, feed[r]:] == CANARY), (call, r, "written past the row's outputs")
            assert feed[r] or gain[r] == 1.0, (call, r)
            pieces[r].append(out[r, :feed[r]])
            at[r] += feed[r]
        bad += nonfinite
        mg = np.where(np.array(feed) > 0, np.minimum(mg, gain), mg)      # (over the calls that fed the row something)
    for r in range(N_ROWS):
        y = np.concatenate(pieces[r])
        assert len(y) == n[r] == whole[1][r]
        same_bits(y, whole[0][r, :n[r]], ("stream", r))
        assert bad[r] == whole[2][r] and np.float64(mg[r] if n[r] else 1.0).view(np.uint64) == np.float64(whole[3][r]).view(np.uint64), r
    assert whole[2][0] == 2
    gpu_ctx.dyn_stream_close(st)
    gpu_ctx.dyn_free(dyn_set)                                   # close, then free


def test_what_a_live_stream_refuses(gpu_ctx, dev):
    lib = G.load()
    curves = three_curves()
    dyn_set = gpu_ctx.dyn_create(curves)
    for args in [(0, None, 0, None), (2, [0, 3], 0, None), (2, None, 1, None), (2, None, 2, [0, 2])]:
        n_rows, which, n_keys, key_rows = args
        with pytest.raises(G.GrailError):
            gpu_ctx.dyn_stream_open(dyn_set, n_rows, which, n_keys, key_rows)
    plain = gpu_ctx.dyn_stream_open(dyn_set, 2)
    keyed = gpu_ctx.dyn_stream_open(dyn_set, 2, None, 1, [0, 0])
    d_in, d_out, d_key = dev.up(np.zeros(128, np.float32)), dev.up(np.zeros(128, np.float32)), dev.up(np.zeros(64, np.float32))
    d_len = dev.up(np.array([64, 10], np.uint32))
    for st, key, key_stride, word in [(plain, d_key, 64, b"takes no key_dev"), (keyed, None, 64, b"needs key_dev"),
                                      (keyed, d_key, 63, b"key_stride < in_stride"), (keyed, d_out, 64, b"overlaps key_dev")]:
        with pytest.raises(G.GrailError):
            gpu_ctx.dyn_stream_next_async(st, d_in, 64, d_len, d_out, 64, key_dev=key, key_stride=key_stride)
        assert word in lib.grail_last_error(), lib.grail_last_error()
    # a call of no samples needs no key; two rows on the one key, the input its own key's neighbour
    out_len, bad, gain = gpu_ctx.dyn_stream_next(keyed, 2, None, 0, d_len, None, 0)
    assert out_len.tolist() == [0, 0] and gain.tolist() == [1.0, 1.0]
    out_len, bad, gain = gpu_ctx.dyn_stream_next(keyed, 2, d_in, 64, d_len, d_out, 64, key_dev=d_key, key_stride=64)
    assert out_len.tolist() == [64, 10] and bad.tolist() == [0, 0]
    with pytest.raises(G.GrailError):
        gpu_ctx.dyn_free(dyn_set)
    gpu_ctx.dyn_stream_close(plain)
    with pytest.raises(G.GrailError):                           # one stream is still open
        gpu_ctx.dyn_free(dyn_set)
    with pytest.raises(G.GrailError):                           # a closed stream is no stream
        gpu_ctx.dyn_stream_next_async(plain, d_in, 64, d_len, d_out, 64)
    gpu_ctx.dyn_stream_close(keyed)
    gpu_ctx.dyn_free(dyn_set)
    with pytest.raises(G.GrailError):                           # a freed set is no set
        gpu_ctx.dyn_stream_open(dyn_set, 2)
