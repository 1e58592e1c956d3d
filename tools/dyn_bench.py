"""Dynamics of rendered rows at full size: the config-3 batch (65 536 rows x 96 006 samples, 25.2 GB)
rendered once, then in one process on the same buffers
  grail_iir_async   with a filter of S = 2 sections (the yardstick: the same shape of kernel, about the same arithmetic),
  grail_dyn_async   self-keyed (8 B a sample) with a soft-knee compressor on the peak detector,
  grail_dyn_async   keyed (12 B a sample): row u listens to row u + n / 2 of the same buffer, key_len_dev the rows' lengths,
beside the time HBM needs for 8 B a sample at the 6.29 TB/s a float4 copy reaches on an MI355X, and a lone row of 10^7 samples
through grail_dyn_async (one lane's serial chain: the figure a wave-per-row form would have to beat) beside grail_iir_async
S = 2 on the same row.  Wall clock around each call and its sync, best of --reps after a warm-up, with the spread (max - min)
/ min of the repeats.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/dyn_bench.py`.  Prints one
line per case and a JSON summary."""
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
    return np.array([G.iir_design(kind, rate, f0, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / (4 * sections))))
                     for k in range(sections)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lone-reps", type=int, default=3)
    ap.add_argument("--lone", type=int, default=10_000_000, help="samples of the lone row (0: skip it)")
    args = ap.parse_args()
    if G.device_count() < 1:
        raise SystemExit("dyn_bench needs a HIP device (no CPU fallback)")
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
    d_key_row = ctx.device_alloc(n * 4)
    ctx.h2d(d_key_row, ((np.arange(n, dtype=np.uint32) + n // 2) % max(n, 1)).astype(np.uint32), n * 4)
    iir_set = ctx.iir_create([butterworth(G.IIR_HIGHPASS, rate, 100.0, 2)])
    curve = (G.dyn_design(G.DYN_COMPRESS, G.DYN_PEAK, -24.0, 3.0, 6.0), G.dyn_ballistics(rate, 5.0, 120.0), G.DYN_PEAK)
    dyn_set = ctx.dyn_create([curve])

    def iir():
        ctx.iir_async(iir_set, d_rows, stride, d_len, n, None, 0, d_out, stride, d_n, d_b)
        ctx.sync()

    def dyn():
        ctx.dyn_async(dyn_set, d_rows, stride, d_len, n, None, d_out, stride, d_n, d_b, d_g)
        ctx.sync()

    def dyn_keyed():
        ctx.dyn_async(dyn_set, d_rows, stride, d_len, n, None, d_out, stride, d_n, d_b, d_g, key_dev=d_rows, key_stride=stride,
                      key_len_dev=d_len, n_keys=n, key_row_dev=d_key_row)
        ctx.sync()

    iir_ms, iir_all = best(iir, args.reps)
    out["cases"]["grail_iir_async_S2"] = {"ms": iir_ms, "ms_all": iir_all, "spread": (max(iir_all) - iir_ms) / iir_ms, "over_hbm": iir_ms / hbm_ms}
    print(f"grail_iir_async S = 2: {iir_ms:.2f} ms (call + sync), spread {100 * (max(iir_all) - iir_ms) / iir_ms:.1f} %; "
          f"{iir_ms / hbm_ms:.2f} x the HBM time of 8 B a sample")
    for name, fn, bytes_a_sample in (("grail_dyn_async", dyn, 8), ("grail_dyn_async_keyed", dyn_keyed, 12)):
        ms, ms_all = best(fn, args.reps)
        spread = (max(ms_all) - ms) / ms
        gains = np.zeros(n, np.float64)
        ctx.d2h(gains, d_g, n * 8)
        out["cases"][name] = {"ms": ms, "ms_all": ms_all, "spread": spread, "over_iir_S2": ms / iir_ms,
                              "over_hbm": ms / (hbm_ms * bytes_a_sample / 8), "smallest_min_gain": float(gains.min())}
        print(f"{name}: {ms:.2f} ms (call + sync), spread {100 * spread:.1f} %; {ms / iir_ms:.2f} x grail_iir_async S = 2, "
              f"{ms / (hbm_ms * bytes_a_sample / 8):.2f} x the HBM time of {bytes_a_sample} B a sample; the smallest min_gain "
              f"{20 * math.log10(max(float(gains.min()), 1e-300)):.2f} dB")
    if args.lone:
        long_n = args.lone
        for p in (d_rows, d_out):
            ctx.device_free(p)
        d_rows, d_out = ctx.device_alloc(long_n * 4), ctx.device_alloc(long_n * 4)
        x = (np.random.default_rng(1).standard_normal(long_n) * 0.1).astype(np.float32)
        ctx.h2d(d_rows, x, long_n * 4)
        ctx.h2d(d_len, np.array([long_n], np.uint32), 4)

        def lone_iir():
            ctx.iir_async(iir_set, d_rows, long_n, d_len, 1, None, 0, d_out, long_n, d_n, d_b)
            ctx.sync()

        def lone_dyn():
            ctx.dyn_async(dyn_set, d_rows, long_n, d_len, 1, None, d_out, long_n, d_n, d_b, d_g)
            ctx.sync()

        ims, ims_all = best(lone_iir, args.lone_reps)
        dms, dms_all = best(lone_dyn, args.lone_reps)
        out["lone_row"] = {"samples": long_n, "iir_S2_ms": ims, "iir_S2_ms_all": ims_all, "dyn_ms": dms, "dyn_ms_all": dms_all}
        print(f"a lone row of {long_n} samples: grail_dyn_async {dms:.1f} ms = {1e6 * dms / long_n:.1f} ns a sample, "
              f"grail_iir_async S = 2 {ims:.1f} ms = {1e6 * ims / long_n:.1f} ns a sample")
    ctx.dyn_free(dyn_set)
    ctx.iir_free(iir_set)
    for p in (d_g, d_b, d_n, d_key_row, d_rows, d_out, d_len):
        ctx.device_free(p)
    b.free()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
