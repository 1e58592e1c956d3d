"""Recursive filtering of rendered rows at full size: the config-3 batch (65 536 rows x 96 006 samples,
25.2 GB) rendered once, then on the same buffer
  grail_iir_async             with filters of S = 1, 2, 4, 8 sections (one lane per row, the rows written back: 8 B a sample),
  grail_biquad_blocked_async     with the same filters at S = 2 and 8 (one lane per block of 1024 steps, the
                              recurrence run twice, 16 S' bytes of scratch a block: with this many rows the serial call wins),
  grail_loudness_async        (the same recurrence at S = 2 with no stores: the first yardstick),
beside the time HBM needs for 8 B a sample at the 6.29 TB/s a float4 copy reaches on an MI355X (the second yardstick), and
a lone row of 10^7 samples at S = 2 and 8, through both calls in turn on the same buffer (one lane's serial work against
9 766 lanes'; the blocked call is held to 50 x the serial one's pace there, and the two outputs are compared).  Wall clock around each call and its sync, best of --reps after
a warm-up, with the spread (max - min) / min of the repeats.  Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/iir_bench.py`.  Prints one line per case and a JSON summary."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "grail-rs_amd"))

import grail_hip as G                      # noqa: E402
from grail_hip import workload as W        # noqa: E402

HBM_BYTES_PER_S = 6.29e12                  # a float4 copy on an MI355X (8.0 TB/s on paper)


def best(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return min(ms), ms


def butterworth(kind, rate, f0, sections):
    """order 2 * sections, by the header's recipe"""
    return np.array([G.iir_design(kind, rate, f0, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / (4 * sections))))
                     for k in range(sections)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sections", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--blocked-sections", type=int, nargs="*", default=[2, 8], help="the S the blocked call runs at on the batch")
    ap.add_argument("--lone-sections", type=int, nargs="*", default=[2, 8])
    ap.add_argument("--lone-reps", type=int, default=5)
    ap.add_argument("--lone", type=int, default=10_000_000, help="samples of the lone row (0: skip it)")
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("iir_bench needs a HIP device (no CPU fallback)")
    ctx = G.Context(0)
    ctx.set_voices(W.single_voice())
    rate = int(W.SAMPLE_RATE)
    n = args.utts
    segs, offs, vids, seeds = W.make_batch(n)
    stride = W.max_samples()
    b = ctx.upload(segs, offs, vids, seeds)
    d_rows, d_len = ctx.device_alloc(n * stride * 4), ctx.device_alloc(n * 4)
    d_out = ctx.device_alloc(n * stride * 4)
    b.synthesize_async(d_rows, stride, d_len)
    ctx.sync()
    lens = np.zeros(n, np.uint32)
    ctx.d2h(lens, d_len, n * 4)
    samples = float(lens.astype(np.float64).sum())
    hbm_ms = 1e3 * samples * 8 / HBM_BYTES_PER_S
    print(f"{n} rows x {int(lens.max())} samples = {samples * 4 / 1e9:.2f} GB; 8 B a sample at {HBM_BYTES_PER_S / 1e12:.2f} TB/s: {hbm_ms:.2f} ms")
    out = {"rows": n, "samples_per_row": int(lens.max()), "samples": samples, "hbm_ms_8B_a_sample": hbm_ms, "cases": {}}
    d_g, d_b, d_n = ctx.device_alloc(n * 8), ctx.device_alloc(n * 4), ctx.device_alloc(n * 4)

    def loudness():
        ctx.loudness_async(d_rows, stride, d_len, n, rate, None, d_g, None, 0, d_b)
        ctx.sync()

    loud_ms, loud_all = best(loudness, args.reps)
    out["cases"]["grail_loudness_async"] = {"ms": loud_ms, "ms_all": loud_all, "spread": (max(loud_all) - loud_ms) / loud_ms}
    print(f"grail_loudness_async: {loud_ms:.2f} ms (call + sync), spread {100 * (max(loud_all) - loud_ms) / loud_ms:.1f} %")
    for S in args.sections:
        iir_set = ctx.iir_create([butterworth(G.IIR_HIGHPASS, rate, 100.0, S)])

        def iir():
            ctx.iir_async(iir_set, d_rows, stride, d_len, n, None, 0, d_out, stride, d_n, d_b)
            ctx.sync()

        ms, ms_all = best(iir, args.reps)
        spread = (max(ms_all) - ms) / ms
        out["cases"][f"grail_iir_async_S{S}"] = {"ms": ms, "ms_all": ms_all, "spread": spread, "over_loudness": ms / loud_ms,
                                                 "over_hbm": ms / hbm_ms, "binary64_ops_a_sample": 9 * S}
        print(f"grail_iir_async S = {S}: {ms:.2f} ms (call + sync), spread {100 * spread:.1f} %; {ms / loud_ms:.2f} x grail_loudness_async, "
              f"{ms / hbm_ms:.2f} x the HBM time of 8 B a sample; {9 * S * samples / (ms * 1e-3) / 1e12:.2f} T binary64 operations a second")
        if S in args.blocked_sections:
            def blocked():
                ctx.iir_blocked_async(iir_set, d_rows, stride, d_len, n, None, 0, d_out, stride, d_n, d_b)
                ctx.sync()

            bms, bms_all = best(blocked, args.reps)
            out["cases"][f"grail_biquad_blocked_async_S{S}"] = {"ms": bms, "ms_all": bms_all, "spread": (max(bms_all) - bms) / bms,
                                                             "over_serial": bms / ms}
            print(f"grail_biquad_blocked_async S = {S}: {bms:.2f} ms (call + sync), spread {100 * (max(bms_all) - bms) / bms:.1f} %; "
                  f"{bms / ms:.2f} x grail_iir_async")
        ctx.iir_free(iir_set)
    if args.lone:
        long_n = args.lone
        for p in (d_rows, d_out):
            ctx.device_free(p)
        d_rows, d_out = ctx.device_alloc(long_n * 4), ctx.device_alloc(long_n * 4)
        x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
        ctx.h2d(d_rows, x, long_n * 4)
        ctx.h2d(d_len, np.array([long_n], np.uint32), 4)
        d_out2 = ctx.device_alloc(long_n * 4)
        out["lone_row"] = {"samples": long_n, "cases": {}}
        for S in args.lone_sections:
            iir_set = ctx.iir_create([butterworth(G.IIR_HIGHPASS, rate, 100.0, S)])

            def lone():
                ctx.iir_async(iir_set, d_rows, long_n, d_len, 1, None, 0, d_out, long_n, d_n, d_b)
                ctx.sync()

            def lone_blocked():
                ctx.iir_blocked_async(iir_set, d_rows, long_n, d_len, 1, None, 0, d_out2, long_n, d_n, d_b)
                ctx.sync()

            ms, ms_all = best(lone, args.lone_reps)
            bms, bms_all = best(lone_blocked, args.lone_reps)
            ys, yb = np.zeros(long_n, np.float32), np.zeros(long_n, np.float32)
            ctx.d2h(ys, d_out, long_n * 4)
            ctx.d2h(yb, d_out2, long_n * 4)
            differ = int(np.count_nonzero(ys.view(np.uint32) != yb.view(np.uint32)))
            apart = float(np.max(np.abs(ys.astype(np.float64) - yb.astype(np.float64))) / np.max(np.abs(ys)))
            out["lone_row"]["cases"][f"S{S}"] = {"serial_ms": ms, "serial_ms_all": ms_all, "blocked_ms": bms, "blocked_ms_all": bms_all,
                                                 "speedup": ms / bms, "outputs_that_differ": differ, "largest_difference_of_peak": apart}
            print(f"a lone row of {long_n} samples, S = {S}: grail_iir_async {ms:.1f} ms = {1e6 * ms / long_n:.1f} ns a sample, "
                  f"grail_biquad_blocked_async {bms:.2f} ms = {1e6 * bms / long_n:.2f} ns a sample: {ms / bms:.0f} x; {differ} of the "
                  f"binary32 outputs differ, by {apart:.2e} of the peak at most")
            ctx.iir_free(iir_set)

        def lone_loudness():
            ctx.loudness_async(d_rows, long_n, d_len, 1, rate, None, d_g, None, 0, d_b)
            ctx.sync()

        lms, _ = best(lone_loudness, 2)
        out["lone_row"]["loudness_ms"] = lms
        print(f"grail_loudness_async on the lone row: {lms:.1f} ms")
        ctx.device_free(d_out2)
    for p in (d_g, d_b, d_n, d_rows, d_out, d_len):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
