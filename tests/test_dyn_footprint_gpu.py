"""grail_dyn_async and grail_dyn_stream_next_async store nothing outside their rows' outputs: the method of
tests/test_store_footprint_gpu.py on the eight instantiations of dyn_kernel (16-byte and 4-byte paths, self-keyed and keyed,
rows and streams).  The output buffer holds a canary bit pattern everywhere: GUARD rows in front of the first row and behind
the last, the words in front of a shifted base, behind every row's n_out up to its stride, the whole of a refused row and of a
row of no samples; 64 words of it lie on either side of out_len, nonfinite and min_gain.  After the call every canary word is
as it was, and the rows themselves are the model's."""
import ctypes as C

import numpy as np
import pytest

import dyn_model as M
import grail_hip as G
from test_dyn_gpu import audio, same_bits, three_curves
from test_levels_gpu import Dev, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
CANARY_BITS = 0xC0DEFACE                         # (a float32 of about -7: no output of these rows)
GUARD_ROWS = 2
PAD = 64
N_ROWS = 67                                      # a whole wave and three rows
LENGTHS = [0, 1, 3, 63, 64, 65, 127, 128, 129, 200, 130, 61]


def guarded(dev, n_words):
    """a device array of n_words words with PAD canary words on either side -> (pointer to the array itself, read-back)"""
    base = dev.up(np.full(n_words + 2 * PAD, CANARY_BITS, np.uint32))

    def words():
        return dev.down(base, n_words + 2 * PAD, np.uint32)
    return C.c_void_p(base.value + 4 * PAD), words


# (stride, base offset in words, out_stride): the 16-byte path, the 4-byte path, and outputs cut inside the rows (which a stream
# never does: its out_stride is at least its in_stride)
SHAPES = {"vec": (256, 0, 256), "scalar": (201, 1, 203), "cut": (256, 0, 100)}
CASES = [(stream, keyed, shape) for stream in (False, True) for keyed in (False, True) for shape in SHAPES if not (stream and shape == "cut")]


@pytest.mark.parametrize("stream,keyed,shape", CASES,
                         ids=[f"{'stream' if s else 'rows'}-{'keyed' if k else 'self-keyed'}-{shape}" for s, k, shape in CASES])
def test_no_store_outside_the_rows_outputs(gpu_ctx, dev, stream, keyed, shape):
    stride, offset, out_stride = SHAPES[shape]
    rng = np.random.default_rng(stride + 2 * keyed + stream)
    curves = three_curves()
    rows = [audio(LENGTHS[i % len(LENGTHS)], rng) for i in range(N_ROWS)]
    which = [int(v) for v in rng.integers(0, 3, N_ROWS)]
    if not stream:
        which[5] = 7                                            # a refused row: nothing of it is written
    keys = [audio(200, rng) for _ in range(N_ROWS)] if keyed else None
    key_lens = [len(x) for x in rows] if keyed else None        # (a stream's key is as long as the row it drives)
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
    st = None
    try:
        if stream:
            st = gpu_ctx.dyn_stream_open(dyn_set, N_ROWS, which, N_ROWS if keyed else 0)
            gpu_ctx.dyn_stream_next_async(st, d_in, stride, d_len, d_out, out_stride, d_out_len, d_bad, d_gain, key_dev=d_key,
                                          key_stride=stride)
        else:
            gpu_ctx.dyn_async(dyn_set, d_in, stride, d_len, N_ROWS, dev.up(np.array(which, np.uint32)), d_out, out_stride, d_out_len,
                              d_bad, d_gain, key_dev=d_key, key_stride=stride, key_len_dev=d_key_len, n_keys=N_ROWS if keyed else 0)
        gpu_ctx.sync()
        buf = dev.down(d_buf, total, np.uint32)
        out_len, bad, gain = read_len(), read_bad(), read_gain()
    finally:
        if st is not None:
            gpu_ctx.dyn_stream_close(st)
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
    assert stream or want[5][1] == M.REFUSED
