"""Meter streams at size, in the style of tools/limiter_bench.py.
  --step whole  the config-3 batch (65 536 rows x 96 006 samples at 48 kHz, 25.2 GB) rendered once, then on the same buffer, in
                the same process: grail_loudness_async (loudness_hops_kernel<true>, whose file and code object are the parent
                commit's) and one `next` call of a meter stream that feeds every row whole, in lockstep
                (meter_stream_hops_kernel<true>, the wave-uniform walk, then the call's true peak and the advance).  The hop
                sums of the two are compared.  Wall clock around each call and its sync, best of --reps after a warm-up; kernel
                times: run under `rocprofv3 --kernel-trace --stats -- python tools/meter_stream_bench.py --step whole`.
  --step live   4 096 rows fed in calls of 480 samples (10 ms at 48 kHz): call + sync of `next` and of `read`, beside
                grail_limit_stream_next_async on the same chunks.  Three small launches a call: latency, not throughput.
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

RATE = 48000
H = RATE // 10


def best(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), ms


def whole_step(ctx, args):
    ctx.set_voices(W.single_voice())
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * 4)
    b.synthesize_async(d_rows, stride, d_len)
    ctx.sync()
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    hs = (stride + H - 1) // H
    d_hops, d_shops = ctx.device_alloc(n * hs * 8), ctx.device_alloc(n * hs * 8)
    d_gated, d_bad, d_nh, d_tp = ctx.device_alloc(n * 8), ctx.device_alloc(n * 4), ctx.device_alloc(n * 4), ctx.device_alloc(n * 8)
    out = {"step": "whole", "rows": n, "samples_per_row": int(lens.max()), "cases": {}}

    def one_shot():
        ctx.loudness_async(d_rows, stride, d_len, n, RATE, None, d_gated, d_hops, hs, d_bad)
        ctx.sync()

    ms, ms_all = best(one_shot, args.reps)
    out["cases"]["grail_loudness_async"] = {"ms": ms, "ms_all": ms_all}
    print(f"grail_loudness_async: {ms:.2f} ms (call + sync: hops and gate)")
    runs = []
    for rep in range(args.reps + 1):
        ms_ = ctx.meter_stream_open(n, RATE, hs)
        ctx.sync()
        t0 = time.perf_counter()
        ms_.next_async(d_rows, stride, d_len, d_shops, hs, d_nh, d_tp, d_bad)
        ctx.sync()
        if rep:
            runs.append(1e3 * (time.perf_counter() - t0))
        if rep == args.reps:
            integrated = ms_.read()[0]
        ms_.close()
    out["cases"]["meter stream next (whole rows)"] = {"ms": min(runs), "ms_all": runs}
    print(f"meter stream, one `next` call of whole rows: {min(runs):.2f} ms (call + sync: hops, true peak, advance)")
    a, c = np.zeros((n, hs)), np.zeros((n, hs))
    ctx.d2h(a, d_hops, a.nbytes)
    ctx.d2h(c, d_shops, c.nbytes)
    gated = np.zeros(n)
    ctx.d2h(gated, d_gated, n * 8)
    differ = sum(int(not np.array_equal(a[u, :lens[u] // H].view(np.uint64), c[u, :lens[u] // H].view(np.uint64))) for u in range(n))
    differ += int(np.count_nonzero(gated.view(np.uint64) != integrated.view(np.uint64)))
    out["rows_that_differ"] = differ
    print(f"rows whose hop sums or gated mean square differ between the two: {differ}")
    assert differ == 0
    # The two hop kernels in turn, each right behind the same neighbour: the stream's hop kernel of one call runs behind the true
    # peak kernel of the call before (16 ms of dense binary64), the one-shot kernel above behind its own kind.  Here the
    # one-shot call is put behind a stream call too, so that the kernel trace shows both behind the same 16 ms.
    turns = {"meter stream next": [], "grail_loudness_async behind it": []}
    for rep in range(args.reps):
        ms_ = ctx.meter_stream_open(n, RATE, hs)
        ctx.sync()
        t0 = time.perf_counter()
        ms_.next_async(d_rows, stride, d_len, d_shops, hs, d_nh, d_tp, d_bad)
        ctx.sync()
        t1 = time.perf_counter()
        ctx.loudness_async(d_rows, stride, d_len, n, RATE, None, d_gated, d_hops, hs, d_bad)
        ctx.sync()
        t2 = time.perf_counter()
        ms_.close()
        turns["meter stream next"].append(1e3 * (t1 - t0))
        turns["grail_loudness_async behind it"].append(1e3 * (t2 - t1))
    out["in_turn_ms"] = turns
    print("in turn (call + sync): " + "; ".join(f"{k} {min(v):.2f} .. {max(v):.2f} ms" for k, v in turns.items()))
    for p in (d_rows, d_len, d_hops, d_shops, d_gated, d_bad, d_nh, d_tp):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


def live_step(ctx, args):
    n, chunk, calls = args.rows, 480, args.calls
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.5, 0.5, (n, chunk)).astype(np.float32)
    d_in, d_len, d_out = ctx.device_alloc(x.nbytes), ctx.device_alloc(n * 4), ctx.device_alloc(n * 512 * 4)
    ctx.h2d(d_in, x, x.nbytes)
    ctx.h2d(d_len, np.full(n, chunk, np.uint32), n * 4)
    d_hops = ctx.device_alloc(n * 8)
    d_res = [ctx.device_alloc(n * 8) for _ in range(5)]
    ms = ctx.meter_stream_open(n, RATE, calls * chunk // H + 2)
    ls = ctx.limit_stream_open(n, 0.4, 8)
    times = {"meter next": [], "meter read": [], "limit next": []}
    for k in range(calls + 10):
        t0 = time.perf_counter()
        ms.next_async(d_in, chunk, d_len, d_hops, 1, d_res[0], d_res[1], d_res[2])
        ctx.sync()
        t1 = time.perf_counter()
        ms.read_async(*d_res)
        ctx.sync()
        t2 = time.perf_counter()
        ls.next_async(d_in, chunk, d_len, d_out, 512, d_res[0], d_res[1], d_res[2], d_res[3])
        ctx.sync()
        t3 = time.perf_counter()
        if k >= 10:
            for name, dt in zip(times, (t1 - t0, t2 - t1, t3 - t2)):
                times[name].append(1e3 * dt)
    hops = ms.read()[4]
    assert int(hops[0]) == (calls + 10) * chunk // H
    out = {"step": "live", "rows": n, "chunk": chunk, "calls": calls, "cases": {}}
    for name, v in times.items():
        out["cases"][name] = {"median_ms": float(np.median(v)), "min_ms": min(v), "p90_ms": float(np.percentile(v, 90))}
        print(f"{name}: median {np.median(v):.3f} ms, min {min(v):.3f}, 90th percentile {np.percentile(v, 90):.3f} (call + sync, {n} rows x {chunk})")
    ms.close()
    ls.close()
    for p in [d_in, d_len, d_out, d_hops] + d_res:
        ctx.device_free(p)
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["whole", "live"], default="whole")
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("meter_stream_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    return whole_step(ctx, args) if args.step == "whole" else live_step(ctx, args)


if __name__ == "__main__":
    main()
