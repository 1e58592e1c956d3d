"""True peak of rendered rows at full size: the config-3 batch (65 536 rows x 96 006 samples, 25.2 GB)
rendered once, then on the same buffer, in the same process,
  grail_true_peak_async       (one wave per row and chunk of 4 096 output times through the 4 x 12 taps, then the fold),
  grail_levels_async          (the row totals of §4.9: one read of every sample, one multiply-add a sample),
  grail_loudness_async        (§4.10: one lane per row through the two biquads),
beside one exact rendering of the batch (the headline kernel), grail_batch_mix_leveled_limited of the babble case in
GRAIL_LEVEL_LOUDNESS against grail_batch_mix_leveled of the same items, and a lone row of 10^7 samples (time is parallel:
it fills the device).  Wall clock around each call and its sync, best of --reps after a warm-up; TB/s of the rows' bytes.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/true_peak_bench.py`; bytes fetched: under
`rocprofv3 --pmc FETCH_SIZE -- python tools/true_peak_bench.py --only-true-peak` (a run of its own).  Prints one line per
case and a JSON summary."""
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
    ap.add_argument("--only-true-peak", action="store_true", help="render, then grail_true_peak_async alone (for a counter run)")
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("true_peak_bench needs a HIP device (no CPU fallback)")
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

    def true_peak():
        ctx.true_peak_async(d_rows, stride, d_len, n, d_g, d_b)
        ctx.sync()

    ms, ms_all = best(true_peak, args.reps)
    report("grail_true_peak_async", ms, ms_all)
    fma = 48.0 * nbytes / 4
    print(f"  48 binary64 multiply-adds a sample: {fma / 1e9:.1f} G of them = {2 * fma / (ms * 1e-3) / 1e12:.1f} TFLOP/s")
    if not args.only_true_peak:
        d_out = [ctx.device_alloc(n * k) for k in (8, 4, 4)]

        def totals():
            ctx.levels_async(d_rows, stride, d_len, n, *d_out)
            ctx.sync()

        def loudness():
            ctx.loudness_async(d_rows, stride, d_len, n, rate, None, d_g, None, 0, d_b)
            ctx.sync()

        report("grail_levels_async", *best(totals, args.reps))
        report("grail_loudness_async", *best(loudness, args.reps))
        for p in d_out:
            ctx.device_free(p)
        item_rows, item_tracks, item_offs, gains, n_tracks, track_len = W.mix_case("babble", lens)
        track_stride = (track_len + 63) // 64 * 64
        d_t = ctx.device_alloc(n_tracks * track_stride * 4)
        level_db = np.random.default_rng(5).uniform(-36.0, -14.0, len(item_rows)).astype(np.float32)
        leveled, _ = best(lambda: b.mix_leveled(item_rows, item_offs, level_db, d_t, track_stride, n_tracks, track_len,
                                                item_tracks=item_tracks, mode=G.LEVEL_LOUDNESS), 3)
        limited_items = []
        limited, _ = best(lambda: limited_items.append(b.mix_leveled_limited(item_rows, item_offs, level_db, d_t, track_stride, n_tracks,
                                                                     track_len, item_tracks=item_tracks, mode=G.LEVEL_LOUDNESS,
                                                                     ceiling_db=-10.0)[3]), 3)
        out["batch_mix_leveled_loudness_ms"] = leveled
        out["batch_mix_leveled_limited_loudness_ms"] = limited
        print(f"grail_batch_mix_leveled_limited (loudness, babble, ceiling -10 dBTP: {limited_items[-1]} of {len(item_rows)} items "
              f"limited): {limited:.2f} ms against grail_batch_mix_leveled {leveled:.2f} ms = +{limited - leveled:.2f} ms")
        ctx.device_free(d_t)
        # a lone long row: time is parallel, so it fills the device
        long_n = 10_000_000
        ctx.device_free(d_rows)
        d_rows = ctx.device_alloc(long_n * 4)
        x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
        ctx.h2d(d_rows, x, long_n * 4)
        ctx.h2d(d_len, np.array([long_n], np.uint32), 4)

        def lone():
            ctx.true_peak_async(d_rows, long_n, d_len, 1, d_g, d_b)
            ctx.sync()

        ms, _ = best(lone, 5)
        out["lone_row_1e7_ms"] = ms
        print(f"a lone row of {long_n} samples: {ms:.3f} ms = {1e6 * ms / long_n:.3f} ns a sample")
    for p in (d_g, d_b, d_rows, d_len):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
