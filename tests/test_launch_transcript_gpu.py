"""What the host code between a batch and its kernel launches decides, recorded on the device: the real upload (length order,
row groups, length bounds), the cached plans, the packed launch tables, streams that borrow or own a batch.  Small shapes:
a device planned as four compute units (one round of the one-lane kernels is 1 024 rows) and utterances of 2 - 6 phonemes of
10 - 50 ms.  One line per launch: the read-only "last_launch_*" options, the kernel the context names, a sha256 over the
rows' on-device digests (grail_batch_digest) and over their lengths.  tests/golden/launch_transcript.txt is what the library
answered while a batch was one struct of facts, raw device pointers and caches; host code that is not meant to move a plan
or a bit must repeat it byte for byte (exact digests are the reference's bits; tolerance-mode digests follow the kernel
family, so equality shows the family did not move).  Run as a script, the module writes the transcript (to the path given)."""
import hashlib
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "grail-rs_amd"), os.path.join(_root, "tests")]

import grail_hip as G
from grail_hip import workload as W

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_transcript.txt")
LAST = ("fast", "blocks", "formants", "lanes", "pipelined", "chunks", "packed")
GRID_OPTIONS = ("row_groups", "packed_launch_order", "arithmetic", "lanes_per_utterance")
CUS, OTHER_CUS = 4, 8


def _voices():
    """generic() (formants 5 - 8 silent: the lean families) and seven presets with all eight formants live"""
    return W.single_voice() + W.preset_voices(7)


def _short_rows(n, seed, n_voices):
    """n utterances of 2 - 6 phonemes of 10 - 50 ms (blends of 8 - 25 ms, any length), a leading Silence"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(2, 7, n)
    offs = np.zeros(n + 1, dtype=np.uint32)
    offs[1:] = np.cumsum(counts)
    k = int(offs[-1])
    segs = np.zeros(k, dtype=G.PHONEME_DTYPE)
    segs["phoneme"] = rng.choice([G.PH_A, G.PH_E, G.PH_SILENCE, G.PH_STOP], k, p=[.4, .4, .12, .08])
    segs["phoneme"][offs[:-1]] = G.PH_SILENCE
    segs["length"] = rng.uniform(0.01, 0.05, k).astype(np.float32)
    segs["blend_length"] = rng.uniform(0.008, 0.025, k).astype(np.float32)
    segs["frequency"] = (rng.uniform(90, 220, k) / W.SAMPLE_RATE).astype(np.float32)
    vids = (np.arange(n) % n_voices).astype(np.uint32)
    seeds = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    return segs, offs, vids, seeds


def _batches(voices):
    """(a) 64 aligned phoneme rows; (b) 2 500 ragged phoneme rows of voice 0, five of them rows the lean families cannot
    take; (c) 600 ragged rows of caller-built elems over the eight voices"""
    import footprint as F
    a = W.make_batch(64, length=0.03125, blend_length=0.03125)
    b = _short_rows(2500, 31, 1)
    segs, offs = b[0], b[1]
    segs["length"][offs[7] + 1] = 0.0                                   # a zero-length segment
    segs["length"][offs[1203] + 1] = 0.0
    segs["length"][offs[400] + 1] = np.float32(1.0 / W.SAMPLE_RATE)     # a one-sample segment
    segs["length"][offs[2499] + 1] = np.float32(1.0 / W.SAMPLE_RATE)
    segs["frequency"][offs[1800] + 1] = np.float32(1e-30)               # a pitch the safe window does not hold
    c = _short_rows(600, 32, 8)
    elems = F.as_sequence_elems(voices, c[0], c[1], c[2])
    return a, b, (list(elems), c[1], c[2], c[3])


def _sha(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()[:24]


def _line(ctx, what, d_out, stride, d_len, n):
    """the launch just queued on ctx, synchronised and told"""
    ctx.sync()
    sums, maxabs, bad = ctx.digest(d_out, stride, d_len, n)
    lens = np.zeros(n, dtype=np.uint32)
    ctx.d2h(lens, d_len, lens.nbytes)
    last = " ".join(f"{k}={ctx.get_option('last_launch_' + k)}" for k in LAST)
    return (f"{what}: {last} kernel={ctx.last_kernel_name()} digest={_sha(sums, maxabs, bad)} "
            f"lens={_sha(lens)} samples={int(lens.sum())}")


def transcript(ctx):
    voices = _voices()
    a, b, c = _batches(voices)
    lines = []
    other = G.Context(0)
    saved = {k: ctx.get_option(k) for k in GRID_OPTIONS + ("assume_compute_units",)}
    bufs = []
    try:
        ctx.set_voices(voices)
        other.set_voices(voices)
        ctx.set_option("assume_compute_units", CUS)
        other.set_option("assume_compute_units", OTHER_CUS)

        def render(name, batch, cells, with_other):
            n = batch.n_utt
            stride = (int(batch.lengths().max()) + 64 + 63) // 64 * 64           # every row ends inside its stride
            d_out, d_len = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * 4)
            bufs.extend([d_out, d_len])
            for cell in cells:
                for k, v in zip(GRID_OPTIONS, cell):
                    ctx.set_option(k, v)
                    other.set_option(k, v)
                tag = f"{name} " + " ".join(f"{k}={v}" for k, v in zip(GRID_OPTIONS, cell))
                for who, which in ((ctx, "first"), (other, f"{OTHER_CUS} units"), (ctx, "again")):
                    if who is other and not with_other:
                        continue
                    who.memset(d_out, 0, n * stride * 4)
                    who.memset(d_len, 0, n * 4)
                    load = G.load().grail_batch_synthesize_async
                    G._check(load(who.handle, batch.handle, d_out, stride, d_len))
                    lines.append(_line(who, f"{tag} {which}", d_out, stride, d_len, n))
            return d_out, d_len, stride

        grid = [(rg, pk, ar, ln) for rg in (0, 1, 2) for pk in (0, 1) for ar in (0, 1) for ln in (0, 1)]
        batch_a = ctx.upload(*a)
        try:
            d_out, d_len, stride = render("a", batch_a, [(1, 1, 0, 0), (1, 1, 1, 0)], False)
            for k, v in zip(GRID_OPTIONS, (1, 1, 0, 0)):
                ctx.set_option(k, v)
            # a resumable stream that borrows the batch, a live stream that owns one (with ids and seeds): one pull each
            st = G.Stream(batch_a)
            try:
                ctx.memset(d_len, 0, 64 * 4)
                st.next_async(512, d_out, stride, d_len)
                lines.append(_line(ctx, "a stream, 512 samples", d_out, stride, d_len, 64))
            finally:
                st.close()
            live = G.LiveStream(ctx, 64, a[2], a[3], ring_segments=8)
            try:
                segs, offs = a[0], a[1]
                live.append(np.concatenate([segs[offs[u]:offs[u] + 2] for u in range(64)]),
                            (2 * np.arange(65)).astype(np.uint32))
                ctx.memset(d_len, 0, 64 * 4)
                live.next_async(512, d_out, stride, d_len)
                lines.append(_line(ctx, "a live stream, two segments, 512 samples", d_out, stride, d_len, 64))
            finally:
                live.close()
        finally:
            ctx.sync()
            batch_a.free()
        for name, batch, with_other in (("b", ctx.upload(*b), True), ("c", ctx.upload_elems(*c), False)):
            try:
                render(name, batch, grid, with_other)
            finally:
                ctx.sync()
                other.sync()
                batch.free()
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)
        ctx.sync()
        for p in bufs:
            ctx.device_free(p)
        other.close()
        ctx.set_voices(W.single_voice())
    return "\n".join(lines) + "\n"


def test_every_launch_repeats_the_recorded_transcript(gpu_ctx):
    got = transcript(gpu_ctx)
    recorded = open(GOLDEN).read()
    assert recorded.count("\n") == 4 + 2 + 24 * 3 + 24 * 2
    for x, y in zip(got.splitlines(), recorded.splitlines()):
        assert x == y
    assert got == recorded


if __name__ == "__main__":
    with G.Context(0) as context:
        text = transcript(context)
    with open(sys.argv[1], "w") as f:
        f.write(text)
    print(f"{text.count(chr(10))} lines")
