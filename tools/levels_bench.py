"""Measuring rendered rows on the device at full size: the config-3 batch (65 536 rows x 96 006 samples,
25.2 GB) rendered once, then one read of every sample timed three ways on the same buffer —
  grail_levels_async          (row totals: frames of 4 096, then the fold over a row's frames),
  grail_frame_levels_async    (frames of 480 samples, 201 a row: every frame starts and ends inside a 256-sample chunk),
  grail_batch_digest          (the older helper: one workgroup a row, 4-byte loads; it also allocates and copies back) —
beside grail_mix_async of the babble case (reads and writes), and grail_batch_mix_leveled against grail_batch_mix of the same
items.  Wall clock around each call and its sync, best of --reps after a warm-up; TB/s of the rows' bytes.  Kernel times: run
under `rocprofv3 --kernel-trace --stats -- python tools/levels_bench.py`.  Prints one line per case and a JSON summary."""
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
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("levels_bench needs a HIP device (no CPU fallback)")
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
    nbytes = float(lens.astype(np.float64).sum()) * 4
    print(f"render: {n} rows x {int(lens.max())} samples = {nbytes / 1e9:.2f} GB, kernel {min(render[1:]):.2f} ms")
    out = {"rows": n, "samples_per_row": int(lens.max()), "bytes": nbytes, "render_kernel_ms": min(render[1:]), "cases": {}}

    def report(name, ms, ms_all, moved=nbytes):
        rate = moved / (ms * 1e-3)
        out["cases"][name] = {"ms": ms, "ms_all": ms_all, "bytes": moved, "tb_per_s": rate / 1e12}
        print(f"{name}: {ms:.2f} ms (call + sync), {moved / 1e9:.2f} GB = {rate / 1e12:.2f} TB/s = "
              f"{100 * rate / PEAK:.1f} % of 8 TB/s, {100 * rate / ACHIEVABLE:.1f} % of 6.3 TB/s")

    d_out = [ctx.device_alloc(n * k) for k in (8, 4, 4)]

    def totals():
        ctx.levels_async(d_rows, stride, d_len, n, *d_out)
        ctx.sync()

    report("grail_levels_async", *best(totals, args.reps))
    frames = -(-stride // 480)
    d_fs, d_fp = ctx.device_alloc(n * frames * 8), ctx.device_alloc(n * frames * 4)

    def frames480():
        ctx.frame_levels_async(d_rows, stride, d_len, n, 480, d_fs, d_fp, frames)
        ctx.sync()

    report("grail_frame_levels_async(480)", *best(frames480, args.reps))
    report("grail_batch_digest", *best(lambda: ctx.digest(d_rows, stride, d_len, n), args.reps))
    for p in d_out + [d_fs, d_fp]:
        ctx.device_free(p)
    # the babble mix of the same rows: reads them and writes the tracks
    item_rows, item_tracks, item_offs, gains, n_tracks, track_len = W.mix_case("babble", lens)
    track_stride = (track_len + 63) // 64 * 64
    d_t = ctx.device_alloc(n_tracks * track_stride * 4)

    def mix():
        ctx.mix_async(d_rows, stride, lens, item_rows, item_offs, d_t, track_stride, n_tracks, track_len,
                      item_tracks=item_tracks, item_gains=gains)
        ctx.sync()

    covered = float(np.sum(np.clip(np.minimum(lens[item_rows].astype(np.float64), track_len - item_offs.astype(np.float64)), 0, None)))
    report("grail_mix_async(babble)", *best(mix, args.reps), moved=covered * 4 + float(n_tracks) * track_len * 4)
    level_db = np.random.default_rng(5).uniform(-30.0, -6.0, len(item_rows)).astype(np.float32)
    plain, _ = best(lambda: b.mix(item_rows, item_offs, d_t, track_stride, n_tracks, track_len, item_tracks=item_tracks,
                                  item_gains=gains), 3)
    for name, mode in (("rms", G.LEVEL_RMS), ("peak", G.LEVEL_PEAK), ("active", G.LEVEL_ACTIVE)):
        ms, _ = best(lambda: b.mix_leveled(item_rows, item_offs, level_db, d_t, track_stride, n_tracks, track_len,
                                           item_tracks=item_tracks, mode=mode), 3)
        out[f"batch_mix_leveled_{name}_ms"] = ms
        print(f"grail_batch_mix_leveled ({name}, babble): {ms:.2f} ms against grail_batch_mix {plain:.2f} ms = +{ms - plain:.2f} ms")
    out["batch_mix_babble_ms"] = plain
    ctx.device_free(d_t)
    ctx.device_free(d_rows)
    ctx.device_free(d_len)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
