"""grail_spectrum_async stores nothing outside its rows' frames: the method of tests/test_dyn_footprint_gpu.py on both shapes of
spectrum_kernel (four frames side by side, a wave each: N = 128; a frame a workgroup: N = 512) and both load widths.  Both
output buffers hold a canary bit pattern everywhere: GUARD rows of frames in front of the first row and behind the last, the
frames from a row's n_frames up to frames_stride (which is made larger than any row needs), the whole of a row of no samples;
64 words of it lie on either side of n_frames and nonfinite.  After the call every canary word is as it was and the frames
themselves are the model's: a bin or a band written past a frame's N/2 + 1 or B would have landed on the next frame's first, or,
behind a row's last frame, on a canary."""
import ctypes as C

import numpy as np
import pytest

import spectrum_model as M
from grail_hip import spectrum as S
from test_levels_gpu import Dev, dev  # noqa: F401  (dev is a fixture)
from test_spectrum_gpu import CANARY_BITS, awkward, hand_bands, place

pytestmark = pytest.mark.gpu
GUARD_ROWS = 2
PAD = 64
N_ROWS = 67


def guarded(dev, n_words):
    """a device array of n_words words with PAD canary words on either side -> (pointer to the array itself, read-back)"""
    base = dev.up(np.full(n_words + 2 * PAD, CANARY_BITS, np.uint32))

    def words():
        return dev.down(base, n_words + 2 * PAD, np.uint32)
    return C.c_void_p(base.value + 4 * PAD), words


# (log2n, W, hop, pad, bands, row stride): 13 and 9 frames a row at the most, so two chunks; frames_stride leaves 3 frames spare
SHAPES = {"waves": (7, 100, 37, 50, 13, 480), "block": (9, 512, 128, 256, 20, 1100)}


@pytest.mark.parametrize("layout", ["vec", "scalar"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_no_store_outside_the_rows_frames(gpu_ctx, dev, shape, layout):
    p, W, hop, pad, B, stride = SHAPES[shape]
    offset = 0
    if layout == "scalar":
        stride, offset = stride + 1, 1
    rng = np.random.default_rng(p + offset)
    w = (rng.standard_normal(W)).astype(np.float32)
    bands = hand_bands(rng, (1 << p) // 2, B)
    edges = [0, 1, W - 1, W, W + 1, hop, hop + 1, 8 * hop, 8 * hop + 1, stride, 0]
    rows = [awkward(rng, n) for n in edges + [int(v) for v in rng.integers(0, stride + 1, N_ROWS - len(edges))]]
    rows[-1] = rows[-1][:0]                                     # the last row of the launch has no frame at all
    want = M.spectrum_model(rows, p, w, hop, pad, *bands)
    rows_dev, d_len = place(dev, rows, stride, offset)
    bins, frames_stride = (1 << p) // 2 + 1, M.frames(stride, hop) + 3
    outputs = []
    for each in (bins, B):
        total = (N_ROWS + 2 * GUARD_ROWS) * frames_stride * each
        d_buf = dev.up(np.full(total, CANARY_BITS, np.uint32))
        first = GUARD_ROWS * frames_stride * each
        outputs.append((d_buf, total, first, each, C.c_void_p(d_buf.value + 4 * first)))
    (d_frames, read_frames), (d_bad, read_bad) = guarded(dev, N_ROWS), guarded(dev, N_ROWS)
    spectrum_set = S.create(gpu_ctx, p, w, hop, pad, bands)
    try:
        S.transform_async(gpu_ctx, spectrum_set, rows_dev, stride, d_len, N_ROWS, outputs[0][4], outputs[1][4], frames_stride, d_frames, d_bad)
        gpu_ctx.sync()
        bufs = [dev.down(d_buf, total, np.uint32) for d_buf, total, _, _, _ in outputs]
        n_frames, bad = read_frames(), read_bad()
    finally:
        S.free(gpu_ctx, spectrum_set)
    # the results' neighbours
    for words in (n_frames, bad):
        assert np.all(words[:PAD] == CANARY_BITS) and np.all(words[PAD + N_ROWS:] == CANARY_BITS), "written beside a result array"
    n_frames, bad = n_frames[PAD:PAD + N_ROWS], bad[PAD:PAD + N_ROWS]
    for which, (buf, (_, total, first, each, _)) in enumerate(zip(bufs, outputs)):
        # the rows' neighbours
        assert np.all(buf[:first] == CANARY_BITS), (which, "written in front of the first row")
        assert np.all(buf[first + N_ROWS * frames_stride * each:] == CANARY_BITS), (which, "written behind the last row")
        grid = buf[first:first + N_ROWS * frames_stride * each].reshape(N_ROWS, frames_stride, each)
        for i, t in enumerate(want):
            assert (n_frames[i], bad[i]) == (t[2], t[3]), i
            assert np.all(grid[i, t[2]:] == CANARY_BITS), (which, i, len(rows[i]), "written behind the row's frames")
            assert np.array_equal(grid[i, :t[2]], t[which].view(np.uint32)), (which, i)
    assert want[0][2] == 0 and want[-1][2] == 0 and max(t[2] for t in want) + 3 == frames_stride
