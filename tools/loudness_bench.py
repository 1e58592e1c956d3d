"""K-weighted loudness of rendered rows at full size: the config-3 batch (65 536 rows x 96 006 samples,
25.2 GB) rendered once, then on the same buffer
  grail_loudness_async        (one lane per row through the two biquads, hop sums into the context's scratch, then the gate),
  grail_levels_async          (the row totals of §4.9: one read of every sample, no recurrence),
beside one exact rendering of the batch (the headline kernel), grail_batch_mix_leveled of the babble case in
GRAIL_LEVEL_LOUDNESS against GRAIL_LEVEL_ACTIVE and grail_batch_mix of the same items, and a lone row of 10^7 samples (one
lane's serial work).  grail_loudness_segmented_async (one lane per hop, each hop filtered from three hops before it) runs
beside the serial call on the config-3 rows (its P + 1 passes against one), on the lone row (the acceptance: at least
100 x the serial call measured in the same run) and on 64 tracks of 10 minutes.  Wall clock around each call and its sync, best of --reps after a warm-up; TB/s of the rows' bytes.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/loudness_bench.py`; bytes fetched: under
`rocprofv3 --pmc FETCH_SIZE -- python tools/loudness_bench.py --only-loudness` (a run of its own; --only-segmented for the
segmented call: how much of its four-fold read reaches HBM).  Prints one line per case
and a JSON summary."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grail-rs_amd"))

import grail_hip as G                      # noqa: E402
from grail_hip import workload as W        # noqa: E402


def best(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-loudness", action="store_true", help="render, then grail_loudness_async alone (for a counter run)")
    ap.add_argument("--only-segmented", action="store_true",
                    help="render, then grail_loudness_segmented_async alone (for a counter run)")
    ap.add_argument("--tracks", type=int, default=64, help="finished tracks of --track-seconds for the segmented call")
    ap.add_argument("--track-seconds", type=int, default=600)
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("loudness_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    ctx.set_voices(W.single_voice())
    rate = int(W.SAMPLE_RATE)
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * 4)
    render = []
    for _ in range(3):
        b.synthesize_async(d_rows, stride, d_len)
        ctx.sync()
        render.append(ctx.last_kernel_ms())
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    nbytes = float(lens.astype(np.float64).sum()) * 4
    print(f"render: {n} rows x {int(lens.max())} samples = {nbytes / 1e9:.2f} GB, kernel {min(render[1:]):.2f} ms")
    out = {"rows": n, "samples_per_row": int(lens.max()), "bytes": nbytes, "render_kernel_ms": min(render[1:]), "cases": {}}

    def report(name, ms, ms_all, moved=nbytes):
        r = moved / (ms * 1e-3)
        out["cases"][name] = {"ms": ms, "ms_all": ms_all, "bytes": moved, "tb_per_s": r / 1e12}
        print(f"{name}: {ms:.2f} ms (call + sync), {moved / 1e9:.2f} GB = {r / 1e12:.2f} TB/s; "
              f"{ms / out['render_kernel_ms']:.3f} x the rendering")

    d_g, d_b = ctx.device_alloc(n * 8), ctx.device_alloc(n * 4)

    def loudness():
        ctx.loudness_async(d_rows, stride, d_len, n, rate, None, d_g, None, 0, d_b)
        ctx.sync()

    def segmented():
        ctx.loudness_segmented_async(d_rows, stride, d_len, n, rate, None, d_g, None, 0, d_b)
        ctx.sync()

    if not args.only_segmented:
        report("grail_loudness_async", *best(loudness, args.reps))
    if not args.only_loudness:
        report("grail_loudness_segmented_async", *best(segmented, args.reps))
        if not args.only_segmented:
            ratio = out["cases"]["grail_loudness_segmented_async"]["ms"] / out["cases"]["grail_loudness_async"]["ms"]
            out["segmented_over_serial_config3"] = ratio
            print(f"config-3 rows: the segmented call takes {ratio:.2f} x the serial one ({G.LOUDNESS_WARMUP_HOPS + 1} passes against 1)")
    if not args.only_loudness and not args.only_segmented:
        d_out = [ctx.device_alloc(n * k) for k in (8, 4, 4)]

        def totals():
            ctx.levels_async(d_rows, stride, d_len, n, *d_out)
            ctx.sync()

        report("grail_levels_async", *best(totals, args.reps))
        for p in d_out:
            ctx.device_free(p)
        item_rows, item_tracks, item_offs, gains, n_tracks, track_len = W.mix_case("babble", lens)
        track_stride = (track_len + 63) // 64 * 64
        d_t = ctx.device_alloc(n_tracks * track_stride * 4)
        level_db = np.random.default_rng(5).uniform(-30.0, -6.0, len(item_rows)).astype(np.float32)
        plain, _ = best(lambda: b.mix(item_rows, item_offs, d_t, track_stride, n_tracks, track_len, item_tracks=item_tracks,
                                      item_gains=gains), 3)
        for name, mode in (("active", G.LEVEL_ACTIVE), ("loudness", G.LEVEL_LOUDNESS)):
            ms, _ = best(lambda: b.mix_leveled(item_rows, item_offs, level_db, d_t, track_stride, n_tracks, track_len,
                                               item_tracks=item_tracks, mode=mode), 3)
            out[f"batch_mix_leveled_{name}_ms"] = ms
            print(f"grail_batch_mix_leveled ({name}, babble): {ms:.2f} ms against grail_batch_mix {plain:.2f} ms = +{ms - plain:.2f} ms")
        out["batch_mix_babble_ms"] = plain
        ctx.device_free(d_t)
        # a lone long row: one lane's serial work
        long_n = 10_000_000
        ctx.device_free(d_rows)
        d_rows = ctx.device_alloc(long_n * 4)
        x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
        ctx.h2d(d_rows, x, long_n * 4)
        ctx.h2d(d_len, np.array([long_n], np.uint32), 4)

        def lone():
            ctx.loudness_async(d_rows, long_n, d_len, 1, rate, None, d_g, None, 0, d_b)
            ctx.sync()

        ms, _ = best(lone, 2)
        out["lone_row_1e7_ms"] = ms
        print(f"a lone row of {long_n} samples: {ms:.1f} ms = {1e6 * ms / long_n:.1f} ns a sample")

        def lone_segmented():
            ctx.loudness_segmented_async(d_rows, long_n, d_len, 1, rate, None, d_g, None, 0, d_b)
            ctx.sync()

        seg_ms, seg_all = best(lone_segmented, args.reps)
        out["lone_row_1e7_segmented_ms"], out["lone_row_1e7_segmented_ms_all"] = seg_ms, seg_all
        out["lone_row_1e7_speedup"] = ms / seg_ms
        print(f"the same row, segmented: {seg_ms:.3f} ms = {ms / seg_ms:.0f} x ({long_n // (rate // 10)} lanes; acceptance: 100 x)")
        # finished tracks: --tracks rows of --track-seconds, the same noise in each
        track_n = args.track_seconds * rate
        ctx.device_free(d_rows)
        d_rows = ctx.device_alloc(args.tracks * track_n * 4)
        x = (np.random.default_rng(2).standard_normal(track_n) * 0.1).astype(np.float32)
        for t in range(args.tracks):
            ctx.h2d(G.C.c_void_p(d_rows.value + t * track_n * 4), x, track_n * 4)
        d_tl = ctx.device_alloc(args.tracks * 4)
        ctx.h2d(d_tl, np.full(args.tracks, track_n, np.uint32), args.tracks * 4)
        d_tg, d_tb = ctx.device_alloc(args.tracks * 8), ctx.device_alloc(args.tracks * 4)

        def tracks():
            ctx.loudness_segmented_async(d_rows, track_n, d_tl, args.tracks, rate, None, d_tg, None, 0, d_tb)
            ctx.sync()

        ms, ms_all = best(tracks, args.reps)
        out["tracks"] = {"rows": args.tracks, "seconds": args.track_seconds, "ms": ms, "ms_all": ms_all}
        print(f"{args.tracks} tracks of {args.track_seconds} s, segmented: {ms:.2f} ms (call + sync) = "
              f"{args.tracks * args.track_seconds / (ms * 1e-3):.0f} x real time")
        for p in (d_tl, d_tg, d_tb):
            ctx.device_free(p)
    for p in (d_g, d_b, d_rows, d_len):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
