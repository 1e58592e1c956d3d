"""Mixing on the device at full size: the config-3 batch (65 536 rows x 96 006 samples, 25.2 GB) rendered
once, then grail_mix_async timed on three mixes of its rows (workload.mix_case) —
  (a) concat:  every row end to end on 64 tracks (reads 25.2 GB, writes 25.2 GB),
  (b) babble:  4 096 tracks of 16 rows at random offsets in [0, 0.5 s), random gains,
  (c) stacked: all 65 536 rows on one track at random offsets in [0, 1 s) —
and grail_batch_mix of (b) against grail_batch_synthesize_async of the same batch.  Wall clock around each call and its
sync (host plan, upload and kernel), best of --reps after a warm-up.  Bytes = covered samples x 4 read + track samples x 4
written (x 2 with accumulate).  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/mix_bench.py`.
Prints one line per case and a JSON summary."""
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

PEAK, ACHIEVABLE = 8.0e12, 6.3e12


def covered_samples(item_rows, offs, lens, track_len):
    o = offs.astype(np.float64)
    return float(np.sum(np.clip(np.minimum(lens[item_rows].astype(np.float64), track_len - o), 0, None)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("mix_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    ctx.set_voices(W.single_voice())
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
    render_ms = min(render[1:])
    print(f"render: {n} rows x {int(lens.max())} samples, kernel {render_ms:.2f} ms")
    out = {"rows": n, "samples_per_row": int(lens.max()), "render_kernel_ms": render_ms, "cases": {}}
    for case in ("concat", "babble", "stacked"):
        item_rows, item_tracks, item_offs, gains, n_tracks, track_len = W.mix_case(case, lens)
        track_stride = (track_len + 63) // 64 * 64
        d_t = ctx.device_alloc(n_tracks * track_stride * 4)
        ms = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            ctx.mix_async(d_rows, stride, lens, item_rows, item_offs, d_t, track_stride, n_tracks, track_len,
                          item_tracks=item_tracks, item_gains=gains)
            ctx.sync()
            if rep:
                ms.append(1e3 * (time.perf_counter() - t0))
        ctx.device_free(d_t)
        cov = covered_samples(item_rows, item_offs, lens, track_len)
        nbytes = cov * 4 + float(n_tracks) * track_len * 4
        rate = nbytes / (min(ms) * 1e-3)
        out["cases"][case] = {"ms": min(ms), "ms_all": ms, "tracks": n_tracks, "track_len": track_len, "items": len(item_rows),
                              "bytes": nbytes, "tb_per_s": rate / 1e12, "of_8tbs": rate / PEAK, "of_6p3tbs": rate / ACHIEVABLE,
                              "of_render": min(ms) / render_ms}
        print(f"({case}) {n_tracks} tracks x {track_len} samples, {len(item_rows)} items: {min(ms):.2f} ms (call + sync), "
              f"{nbytes / 1e9:.2f} GB moved = {rate / 1e12:.2f} TB/s = {100 * rate / PEAK:.1f} % of 8 TB/s, "
              f"{100 * rate / ACHIEVABLE:.1f} % of 6.3 TB/s; {min(ms) / render_ms:.3f} x the render")
    # grail_batch_mix of (b) against rendering the batch alone
    item_rows, item_tracks, item_offs, gains, n_tracks, track_len = W.mix_case("babble", lens)
    track_stride = (track_len + 63) // 64 * 64
    d_t = ctx.device_alloc(n_tracks * track_stride * 4)
    alone, both = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        b.synthesize_async(d_rows, stride, d_len)
        ctx.sync()
        alone.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        b.mix(item_rows, item_offs, d_t, track_stride, n_tracks, track_len, item_tracks=item_tracks, item_gains=gains)
        both.append(1e3 * (time.perf_counter() - t0))
    ctx.device_free(d_t)
    out["batch_mix_babble_ms"], out["render_alone_ms"] = min(both[1:]), min(alone[1:])
    print(f"grail_batch_mix (babble): {min(both[1:]):.2f} ms against grail_batch_synthesize_async + sync "
          f"{min(alone[1:]):.2f} ms = {min(both[1:]) / min(alone[1:]):.3f} x")
    ctx.device_free(d_rows)
    ctx.device_free(d_len)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
