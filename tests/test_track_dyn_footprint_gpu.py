"""grail_track_dyn_async stores nothing outside its rows' outputs: the method of tests/test_dyn_footprint_gpu.py on the four
instantiations of track_env_kernel (16-byte and 4-byte paths, self-keyed and keyed), with rows of lengths either side of a
tile of T = TRACK_TILE samples.  The output buffer holds a canary bit pattern everywhere: GUARD rows in front of the first row
and behind the last, the words in front of a shifted base, behind every row's n_out up to its stride, the whole of a refused
row and of a row of no samples; 64 words of it lie on either side of out_len, nonfinite and min_gain.  After the call every
canary word is as it was, and the rows themselves are the model's."""
import ctypes as C

import numpy as np
import pytest

import dyn_model as M
from test_dyn_footprint_gpu import CANARY_BITS, GUARD_ROWS, PAD, guarded
from test_dyn_gpu import audio, same_bits, three_curves
from test_levels_gpu import Dev, dev  # noqa: F401  (dev is a fixture)
from test_track_dyn_gpu import T

pytestmark = pytest.mark.gpu
N_ROWS = 67
LENGTHS = [0, 1, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
# (stride, base offset in words, out_stride): the 16-byte path, the 4-byte path, and outputs cut inside a row's second tile
SHAPES = {"vec": (2 * T + 64, 0, 2 * T + 64), "scalar": (2 * T + 9, 1, 2 * T + 11), "cut": (2 * T + 64, 0, T + 100)}
CASES = [(keyed, shape) for keyed in (False, True) for shape in SHAPES]


@pytest.mark.parametrize("keyed,shape", CASES, ids=[f"{'keyed' if k else 'self-keyed'}-{shape}" for k, shape in CASES])
def test_no_store_outside_the_rows_outputs(gpu_ctx, dev, keyed, shape):
    stride, offset, out_stride = SHAPES[shape]
    rng = np.random.default_rng(stride + 2 * keyed)
    curves = three_curves()
    rows = [audio(LENGTHS[i % len(LENGTHS)], rng) for i in range(N_ROWS)]
    which = [int(v) for v in rng.integers(0, 3, N_ROWS)]
    which[5] = 7                                                # a refused row: nothing of it is written
    keys = [audio(T + 200, rng) for _ in range(N_ROWS)] if keyed else None
    key_lens = [len(x) for x in keys] if keyed else None
    want = M.dyn_model(rows, curves, which, keys=keys, key_lens=key_lens, out_stride=out_stride)
    host = np.full(N_ROWS * stride + offset, np.nan, np.float32)
    for i, x in enumerate(rows):
        host[offset + i * stride:offset + i * stride + len(x)] = x
    d_in = C.c_void_p(dev.up(host).value + 4 * offset)
    d_len = dev.up(np.array([len(x) for x in rows], np.uint32))
    d_key, d_key_len = None, None
    if keyed:
        khost = np.full(N_ROWS * stride + offset, np.nan, np.float32)
        for i, k in enumerate(keys):
            khost[offset + i * stride:offset + i * stride + len(k)] = k
        d_key = C.c_void_p(dev.up(khost).value + 4 * offset)
        d_key_len = dev.up(np.array(key_lens, np.uint32))
    total = (N_ROWS + 2 * GUARD_ROWS) * out_stride + offset
    d_buf = dev.up(np.full(total, CANARY_BITS, np.uint32))
    first = GUARD_ROWS * out_stride + offset
    d_out = C.c_void_p(d_buf.value + 4 * first)
    (d_out_len, read_len), (d_bad, read_bad) = guarded(dev, N_ROWS), guarded(dev, N_ROWS)
    d_gain, read_gain = guarded(dev, 2 * N_ROWS)                # (float64: two words a row)
    dyn_set = gpu_ctx.dyn_create(curves)
    try:
        gpu_ctx.track_dyn_async(dyn_set, d_in, stride, d_len, N_ROWS, dev.up(np.array(which, np.uint32)), d_out, out_stride, d_out_len,
                                d_bad, d_gain, key_dev=d_key, key_stride=stride, key_len_dev=d_key_len, n_keys=N_ROWS if keyed else 0)
        gpu_ctx.sync()
        buf = dev.down(d_buf, total, np.uint32)
        out_len, bad, gain = read_len(), read_bad(), read_gain()
    finally:
        gpu_ctx.dyn_free(dyn_set)
    # the results' neighbours
    for words, n in ((out_len, N_ROWS), (bad, N_ROWS), (gain, 2 * N_ROWS)):
        assert np.all(words[:PAD] == CANARY_BITS) and np.all(words[PAD + n:] == CANARY_BITS), "written beside a result array"
    out_len, bad = out_len[PAD:PAD + N_ROWS], bad[PAD:PAD + N_ROWS]
    gain = gain[PAD:PAD + 2 * N_ROWS].view(np.float64)
    # the rows' neighbours
    assert np.all(buf[:first] == CANARY_BITS), "written in front of the first row"
    assert np.all(buf[first + N_ROWS * out_stride:] == CANARY_BITS), "written behind the last row"
    grid = buf[first:first + N_ROWS * out_stride].reshape(N_ROWS, out_stride)
    for i, (y, n_out, w_bad, w_gain) in enumerate(want):
        assert (out_len[i], bad[i]) == (n_out, w_bad), i
        if n_out == M.REFUSED:
            assert np.all(grid[i] == CANARY_BITS) and np.isnan(gain[i]), (i, "a refused row")
            continue
        assert gain[i].view(np.uint64) == np.float64(w_gain).view(np.uint64), i
        assert np.all(grid[i, n_out:] == CANARY_BITS), (i, len(rows[i]), "written behind the row's outputs")
        same_bits(grid[i, :n_out].view(np.float32), y, i)
        assert not np.any(grid[i, :n_out] == CANARY_BITS), i
    assert want[5][1] == M.REFUSED
